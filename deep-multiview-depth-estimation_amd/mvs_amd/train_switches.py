"""The training switches: every MVS_TRAIN_* environment variable, its words, its default and what it moves.
This module is the only reader of them; the predicates that route a layer (region_train.enabled, bn_train.enabled,
model.conv2d_bwd_mode, ...) are a lookup here plus a condition on the tensor (device_fp32).

The environment is read on every call: tests and tools flip the variables inside one process.

How a value that is not one of the words is taken differs from switch to switch, and is kept as it was when each
switch was added (the ``empty`` and ``strict`` fields); the result of ``read`` is compared by the caller (``is_``,
``names``), so a junk value is simply no word."""
import collections
import os

import torch

Switch = collections.namedtuple("Switch", "name default words kinds empty strict doc")
# words: the values with a meaning.  kinds: for a comma-list switch, the layer kinds a list may name ("hip" = all of
# them, "taps" = none).  empty: what an empty value means -- "default", or "" (taken as it is: no word, no kind).
# strict: any other value raises.

_ROWS = (
    Switch("MVS_TRAIN_LIVE", "1", ("1", "0"), (), "", False,
           "`0`: the regulariser under autograd evaluates the full volume (`forward_full`) instead of its live "
           "regions; anything else is on (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_NARROW", "1", ("1", "0"), (), "", False,
           "`0`: `conv_0_0` / `conv_out` on the per-tap GEMMs instead of the narrow HIP kernels; anything else is "
           "on (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_CONV2D", "taps", ("taps", "miopen"), (), "", False,
           "`miopen` (any value but `taps`): the encoder / refinement Conv2d layers stay on the torch modules "
           "(MIOpen) under autograd (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_CONV2D_FWD", "hip", ("hip", "taps"), (), "", False,
           "`taps` (any value but `hip`): the Conv2d forward on the per-tap GEMMs instead of "
           "`csrc/conv2d_narrow.hip`; acts only under `MVS_TRAIN_CONV2D=taps` (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_CONV2D_BWD", "taps", ("hip", "taps"), (), "default", True,
           "`hip`: the twelve encoder / refinement Conv2d layers take their input and weight gradients from "
           "`csrc/conv2d_bwd.hip` instead of 9 or 25 per-tap GEMMs each; acts only where `MVS_TRAIN_CONV2D=taps` "
           "and `MVS_TRAIN_CONV2D_FWD=hip` do; empty = `taps`, anything else raises (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_REGION_FWD", "s1,t2", ("hip", "taps"), ("s1", "s2", "t2"), "", False,
           "which region convolutions run their forward on the HIP region kernels: a comma list of `s1` (conv_k_1), "
           "`s2` (stacked conv_k_0), `t2` (deconv_3_0 / deconv_2_0), `hip` (all) or `taps` (none); empty = none. "
           "`s2` stays off by default (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_REGION_BWD", "taps", ("hip", "taps"), ("s1",), "", False,
           "which region convolutions run their backward on HIP kernels as well: a comma list of kinds, `hip` = "
           "every kind that has one (today `s1`: conv_k_1 with 16 / 32 / 64 channels) or `taps`; `s1` takes the "
           "cfg-2 train step from 237 to 215 ms (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_S2_BWD", "taps", ("hip", "taps"), (), "", False,
           "`hip`: the stacked stride-2 convolutions (32 -> 16 + 32 + 64) take their input and weight gradients "
           "from HIP kernels that read the NCDHW volume in place (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_T2_BWD", "taps", ("hip", "taps"), (), "", False,
           "`hip`: `deconv_3_0` / `deconv_2_0` take their input and weight gradients from HIP kernels that read the "
           "channels-last output gradient in place (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_DECONV1", "taps", ("hip", "taps"), (), "", False,
           "`hip`: `deconv_1_0` (16 -> 8 into the full-size volume) runs its forward, input gradient and weight "
           "gradient on HIP kernels instead of 27 per-tap GEMM passes each (DESIGN.md §3.6)"),
    Switch("MVS_TRAIN_BN", "torch", ("hip", "torch"), (), "", False,
           "`hip`: the ten train-mode BatchNorm + ReLU sites of the live-region regulariser run as one autograd "
           "node each on HIP kernels instead of a dozen elementwise torch passes per site (DESIGN.md §3.6)"),
)
TABLE = collections.OrderedDict((row.name, row) for row in _ROWS)

# Assignments for the tools and tests (tools/train_step_ab.py --switches); the package never reads them.  "all_hip"
# is what the cfg-2 train-step numbers of DESIGN.md §3.6 "with the other switches on" were measured with;
# MVS_TRAIN_REGION_FWD stays at its default there (the stride-2 forward stays on the tap GEMMs, §3.6).
PRESETS = {
    "default": {},
    "all_hip": {"MVS_TRAIN_REGION_BWD": "hip", "MVS_TRAIN_S2_BWD": "hip", "MVS_TRAIN_T2_BWD": "hip",
                "MVS_TRAIN_DECONV1": "hip", "MVS_TRAIN_BN": "hip", "MVS_TRAIN_CONV2D_BWD": "hip"},
}


def read(name):
    """The switch's value in the environment now (its default when unset)."""
    row = TABLE[name]
    v = os.environ.get(name, row.default)
    if v == "" and row.empty == "default":
        v = row.default
    if row.strict and v not in row.words:
        raise ValueError("%s must be %s, got %r" % (name, " or ".join(repr(w) for w in row.words), v))
    return v


def is_(name, word):
    return read(name) == word


def names(name, kind):
    """A comma-list switch names ``kind``: in the list, or the list is "hip"."""
    v = read(name)
    return v == "hip" or (kind is not None and kind in v.split(","))


def accepts(name, value):
    """``value`` is one of the switch's words (or a comma list of its kinds)."""
    row = TABLE[name]
    return value in row.words or (bool(row.kinds) and all(k in row.kinds for k in value.split(",")))


def parse_assignment(text):
    """A preset's name or "NAME=value,NAME=value" -> {name: value} (a comma-list value: "NAME=s1,t2" continues
    until the next NAME=)."""
    if text in PRESETS:
        return dict(PRESETS[text])
    out, last = {}, None
    for part in filter(None, text.split(",")):
        if "=" in part:
            last, v = part.split("=", 1)
            if last not in TABLE:
                raise ValueError("unknown training switch %r (known: %s)" % (last, ", ".join(TABLE)))
            out[last] = v
        elif last is None:
            raise ValueError("expected a preset (%s) or NAME=value,..., got %r" % (", ".join(PRESETS), text))
        else:
            out[last] += "," + part
    return out


def device_fp32(x, grad=False):
    """The tensor condition the switches share: an fp32 tensor on the GPU -- with ``grad``, under autograd too.
    (Today region_train.enabled, bn_train.enabled and d1_applies ask for grad mode; s2_bwd_enabled, t2_bwd_enabled,
    d1_enabled and narrow_train.applies are asked where it is already known.)"""
    return x.is_cuda and x.dtype == torch.float32 and (not grad or torch.is_grad_enabled())
