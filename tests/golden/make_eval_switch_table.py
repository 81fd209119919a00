"""What every eval-path MVS_* variable means, recorded from the code BEFORE mvs_amd/eval_switches.py existed:
eval_switch_table.json.

    python tests/golden/make_eval_switch_table.py          # on a checkout of the PARENT commit; no GPU needed

writes tests/golden/eval_switch_table.json with the commit it ran on ("parent"); tests/test_eval_switches.py
evaluates the same predicates with the code under test and compares.  It uses only names the parent already had,
never eval_switches.

  table    for every variable alone (the others unset) at each of VALUES: every predicate of predicates().
           CostVolumeReg.head_ok / _split_head_ok / _fp32_head_ok are the methods themselves, asked with stand-ins
           for the tensors (they read is_cuda, dtype, dim() and shape only) in the state where everything but the
           switch holds, and in one where a tensor condition fails.  The decisions that are inline in a larger
           function (bound words or None in _forward_live_hip / _forward_live_train_hip / _run_stack, `deferred`
           in MVSNet._forward_one, the glue branch of MVSNet.refine) are restated here word for word (inline_parent)
           with their tensor condition True and False; the test holds the named predicates to them.
           MVSNet().pipeline_chunks and MVSConfig().arithmetic are read off freshly built objects; a ValueError is
           recorded with its message.  "t2 slots" is ops.split_stats_slots of a small transposed split convolution
           (host arithmetic of the library): the parent's library read MVS_T2_LDS itself, the change's gets flags.
"""
import contextlib
import json
import os
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(_HERE))
TABLE = os.path.join(_HERE, "eval_switch_table.json")
_PKG = os.path.join(REPO, "deep-multiview-depth-estimation_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

# the eight variables the package read inline, and MVS_T2_LDS (observable without a GPU through the slot count)
VARIABLES = ("MVS_CV_HEAD", "MVS_SPLIT_HEAD", "MVS_FP32_HEAD", "MVS_REGION_SPLIT", "MVS_CONV2D_F16", "MVS_REFINE_GLUE",
             "MVS_PIPELINE_CHUNKS", "MVS_ARITHMETIC", "MVS_T2_LDS")
# every variable the table of the change names (all unset while another one is varied)
ALL_VARIABLES = VARIABLES + ("MVS_S2_LDS", "MVS_CV_CSPLIT", "MVS_CONV2D_SPLIT")
VALUES = (None, "", "0", "1", "2", "junk", " 2x", "split_f16")   # (" 2x": what atoi takes as 2)
LIVE_N = (20, 32, 40)            # D even, every stride-2 padding odd: the head kernels' geometry
T2_SIZE = (26, 18, 22)           # tests/test_library.py's region: below the size where the LDS kernel is the default
T2_LARGE = (128, 128, 128)       # ... and 2 x 2^21 voxels: at it (no launch: the slot count is host arithmetic)


class Stub:
    """What the predicates read of a tensor."""

    def __init__(self, is_cuda, dtype, shape):
        self.is_cuda, self.dtype, self.shape = is_cuda, dtype, tuple(shape)

    def dim(self):
        return len(self.shape)


class DeferredStub:
    """What CostVolumeReg.head_ok reads of a costvolume.DeferredCostVolume."""

    def __init__(self, is_cuda, n_views):
        self.shape = (2, 32) + LIVE_N
        self.feature_maps = Stub(is_cuda, torch.float32, (2 * n_views, 32) + LIVE_N[1:])
        self.n_views = n_views


def key(v):
    return "<unset>" if v is None else v


@contextlib.contextmanager
def environment(assignment):
    """Exactly ``assignment`` (None = unset) of the eval variables, every other one unset."""
    saved = {k: os.environ.pop(k) for k in ALL_VARIABLES if k in os.environ}
    os.environ.update({k: v for k, v in assignment.items() if v is not None})
    try:
        yield
    finally:
        for k in assignment:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _outcome(fn):
    try:
        return fn()
    except ValueError as e:
        return "ValueError: %s" % e


def inline_parent(state):
    """The five inline decisions as the parent spelled them, their tensor condition being ``state``."""
    return {
        "model.deferred": state and os.environ.get("MVS_CV_HEAD", "0") == "1",
        "model.refine_glue": state and os.environ.get("MVS_REFINE_GLUE", "1") != "0",
        "model.conv2d_words": state and os.environ.get("MVS_CONV2D_F16", "1") != "0",
        "regulariser.bw(eval)": state and os.environ.get("MVS_REGION_SPLIT", "1") != "0",
        "regulariser.bw(train)": state and os.environ.get("MVS_REGION_SPLIT", "1") != "0",
    }


_FIXED = {}


def _reg():
    if not _FIXED:
        from mvs_amd.config import pad_outpad
        from mvs_amd.model import CostVolumeReg
        pad, outpad = pad_outpad(*LIVE_N)
        _FIXED["reg"] = CostVolumeReg(pad=pad, outpad=outpad).eval()
    return _FIXED["reg"]


def predicates(inline=inline_parent):
    """{name: result} of every replaced predicate in the current environment (grad mode off: inference)."""
    from mvs_amd import ops
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    reg = _reg()
    out = {}
    with torch.no_grad():
        for split_f16 in (True, False):
            reg.split_f16 = split_f16
            for is_cuda in (True, False):
                out["head_ok(split_f16=%s,cuda=%s)" % (split_f16, is_cuda)] = bool(reg.head_ok(DeferredStub(is_cuda, 3)))
        reg.split_f16 = True
        out["head_ok(4 views)"] = bool(reg.head_ok(DeferredStub(True, 4)))
        reg.split_f16 = False
    for quads in (8, 4):
        cv = Stub(True, torch.int32, (2, quads) + LIVE_N + (4,))
        out["_split_head_ok(quads=%d)" % quads] = bool(reg._split_head_ok(cv, LIVE_N))
    for dtype in (torch.float32, torch.int32):
        cv = Stub(True, dtype, (2, 8) + LIVE_N + (4,))
        for c4 in (True, False):
            out["_fp32_head_ok(%s,c4=%s)" % (str(dtype).split(".")[1], c4)] = bool(reg._fp32_head_ok(cv, c4, reg.pad))
    for state in (True, False):
        for name, result in inline(state).items():
            out["%s[%s]" % (name, state)] = bool(result)
    out["MVSNet().pipeline_chunks"] = _outcome(lambda: MVSNet().pipeline_chunks)
    out["MVSConfig().arithmetic"] = _outcome(lambda: MVSConfig().arithmetic)
    out["MVSConfig(arithmetic=fp32).arithmetic"] = _outcome(lambda: MVSConfig(arithmetic="fp32").arithmetic)
    for pair in ((64, 32), (32, 16)):
        for per_lane in (False, True):
            for in_bn in (False, True):
                for size in (T2_SIZE, T2_LARGE):
                    name = "t2 slots %d->%d %s per_lane=%s in_bn=%s" % (pair + (size, per_lane, in_bn))
                    out[name] = ops.split_stats_slots(ops.CONV_T2, 2, pair[0], pair[1], size, per_lane, False, in_bn)
    out["s1 slots per_lane=False"] = ops.split_stats_slots(ops.CONV_S1, 2, 16, 16, T2_SIZE)
    out["s1 slots per_lane=True"] = ops.split_stats_slots(ops.CONV_S1, 2, 16, 16, T2_SIZE, True)
    return out


def predicate_table(inline=inline_parent):
    """(records, table): table[variable][value] indexes the list of distinct {predicate: result} records."""
    records, table = [], {}
    for var in VARIABLES:
        for v in VALUES:
            with environment({var: v}):
                rec = predicates(inline)
            if rec not in records:
                records.append(rec)
            table.setdefault(var, {})[key(v)] = records.index(rec)
    return records, table


if __name__ == "__main__":
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True).strip() \
        if os.path.isdir(os.path.join(REPO, ".git")) else os.environ.get("MVS_PINS_PARENT", "")
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    records, table = predicate_table()
    with open(out, "w") as f:
        json.dump({"parent": head, "records": records, "table": table}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records (parent %s)" % (out, len(records), head))
