"""The eval-path switches: every MVS_* environment variable that picks a kernel or a path of the inference
forward, its default, its words, how other values are taken and what it moves.  This module is the only reader of
them (train_switches.py holds the MVS_TRAIN_* ones); the callers ask the predicates below, next to their condition
on the tensors.

The environment is read on every call: tests and tools flip the variables inside one process.

How a value that is not a word is taken differs from switch to switch and is kept as it was when each switch was
added (the ``rule`` field):
  "not 0"    on unless the value is exactly "0": empty and junk are on
  "is 1"     on only for exactly "1": empty and junk are off
  "starts 1" on when the first character is "1" (the library's test, when it read the variable itself)
  "atoi"     the leading integer of the value as C's atoi takes it: empty and junk are 0
  "int"      Python's int(): empty and junk raise its ValueError
  "word"     the value itself; MVSConfig raises on anything but a word
  "library"  not read here: csrc/common.h env_int reads it on every launch (atoi, clamped by the launcher)"""
import collections
import os
import re

Switch = collections.namedtuple("Switch", "name default words rule doc")

_ROWS = (
    Switch("MVS_ARITHMETIC", "fp32", ("fp32", "split_f16"), "word",
           "the arithmetic of an `MVSConfig` built without one: `fp32` (exact) or `split_f16` (the f16 matrix cores "
           "with split operands); anything else raises (DESIGN.md §3.5)"),
    Switch("MVS_CV_HEAD", "0", ("0", "1"), "is 1",
           "`1`: the fused head kernel forms the cost volume on chip inside `conv_0_0` / `conv_1_0` (split_f16, "
           "2-3 views, D even); opt-in, anything else is off (DESIGN.md §3.7)"),
    Switch("MVS_SPLIT_HEAD", "1", ("1", "0"), "not 0",
           "`0`: `conv_0_0` and `conv_1_0` of the split-fp16 path as two kernels instead of one pass over the split "
           "volume; anything else is on (DESIGN.md §3.7)"),
    Switch("MVS_FP32_HEAD", "0", ("0", "1"), "is 1",
           "`1`: the exact-fp32 fused head (`conv_1_0` inside `conv_0_0`'s kernel); measured slower, anything else "
           "is off (DESIGN.md §3.9)"),
    Switch("MVS_REGION_SPLIT", "1", ("1", "0"), "not 0",
           "`0`: the stride-1 and transposed region convolutions of the split-fp16 path on the fp32-MFMA kernels; "
           "anything else is on (DESIGN.md §3.8)"),
    Switch("MVS_CONV2D_F16", "1", ("1", "0"), "not 0",
           "`0`: the encoder / refinement Conv2d layers of the split-fp16 path on the exact-fp32 kernel; anything "
           "else is on (DESIGN.md §3.5)"),
    Switch("MVS_REFINE_GLUE", "1", ("1", "0"), "not 0",
           "`0`: the elementwise steps around the refinement net as torch ops instead of one HIP launch each; "
           "anything else is on (DESIGN.md §5)"),
    Switch("MVS_PIPELINE_CHUNKS", "1", (), "int",
           "chunks of samples an eval forward of B >= 2 issues on streams of their own, read when `MVSNet` is "
           "built; `1` = off, measured slower; not an integer raises (DESIGN.md §3.9)"),
    Switch("MVS_S2_LDS", "0", ("0", "1"), "starts 1",
           "`1`: `ops.conv3d_region` sets `MVS_CONV_S2_LDS` (fp32 `conv_1_0` on the LDS-staged stride-2 kernel); "
           "measured slower (DESIGN.md §3.9)"),
    Switch("MVS_T2_LDS", "1", ("1", "0", "2"), "atoi",
           "`0` / `2`: the split-fp16 transposed region convolutions on the per-lane / the LDS-staged kernel at "
           "every size (`ops` sets `MVS_CONV_PER_LANE` / `MVS_CONV_T2_LDS`); else by output size (DESIGN.md §3.8)"),
    Switch("MVS_CV_CSPLIT", "2", (), "library",
           "read by the library: channel-chunk split (1..8) of the fused cost-volume kernel for small depth "
           "shards (DESIGN.md §3.1)"),
    Switch("MVS_CONV2D_SPLIT", "", (), "library",
           "read by the library: forces the output-channel split (1, 2, 4; capped per layer) of the direct Conv2d "
           "kernel; unset = by grid size (DESIGN.md §5)"),
)
TABLE = collections.OrderedDict((row.name, row) for row in _ROWS)

_ATOI = re.compile(r"[ \t\n\v\f\r]*([+-]?[0-9]+)")


def read(name):
    """The switch's value in the environment now (its default when unset)."""
    row = TABLE[name]
    if row.rule == "library":
        raise KeyError("%s is read by the library, not by the package" % name)
    return os.environ.get(name, row.default)


def on(name):
    """An on / off switch by its rule."""
    v, rule = read(name), TABLE[name].rule
    if rule == "not 0":
        return v != "0"
    if rule == "is 1":
        return v == "1"
    if rule == "starts 1":
        return v[:1] == "1"
    raise KeyError("%s is not an on / off switch" % name)


def cv_head():
    return on("MVS_CV_HEAD")


def split_head():
    return on("MVS_SPLIT_HEAD")


def fp32_head():
    return on("MVS_FP32_HEAD")


def region_split():
    return on("MVS_REGION_SPLIT")


def conv2d_f16():
    return on("MVS_CONV2D_F16")


def refine_glue():
    return on("MVS_REFINE_GLUE")


def s2_lds():
    return on("MVS_S2_LDS")


def t2_lds():
    """0: the per-lane kernel, 2: the LDS-staged kernel, anything else: by output size."""
    m = _ATOI.match(read("MVS_T2_LDS"))
    return int(m.group(1)) if m else 0


def pipeline_chunks():
    return int(read("MVS_PIPELINE_CHUNKS"))


def arithmetic():
    return read("MVS_ARITHMETIC")
