"""What every MVS_TRAIN_* variable means, recorded from the code BEFORE mvs_amd/train_switches.py existed:
train_switch_table.json.

    python tests/golden/make_train_switch_table.py          # on a checkout of the PARENT commit; no GPU needed

writes tests/golden/train_switch_table.json with the commit it ran on ("parent"); tests/test_train_switches.py
evaluates the same predicates and routing decisions with the code under test and compares.  It uses only names the
parent already had (the public predicates, regions._taps, the constants of region_train), never train_switches.

  table    for every variable alone (the ten others unset) at each of VALUES: every predicate of predicates() under
           each of CONTEXTS -- a stand-in for the tensor (the predicates read is_cuda, dtype, dim() and shape only)
           on / off the GPU, with grad mode on / off, and one fp16 stand-in.  A ValueError is recorded with its
           message.  The two reads that were inline in model._run_stack are restated here word for word
           (run_stack_parent); the test holds model.conv2d_train_backends to them.
  routes   the parent's PAIR of decisions per region layer family, composed: the condition in regions.py under which
           the layer goes to the autograd box, and the backends the box entry (s2_box / _S1Valid.forward / t2_box /
           d1_applies) then picked.  One character per geometry: "-" stays on the tap GEMMs / torch, else the digit
           2 * hip_fwd + hip_bwd.  Keys "FWD;BWD[;D1];context", None = unset.
"""
import contextlib
import json
import os
import subprocess
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(_HERE))
TABLE = os.path.join(_HERE, "train_switch_table.json")
_PKG = os.path.join(REPO, "deep-multiview-depth-estimation_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

VARIABLES = ("MVS_TRAIN_LIVE", "MVS_TRAIN_NARROW", "MVS_TRAIN_CONV2D", "MVS_TRAIN_CONV2D_FWD", "MVS_TRAIN_CONV2D_BWD",
             "MVS_TRAIN_REGION_FWD", "MVS_TRAIN_REGION_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_T2_BWD",
             "MVS_TRAIN_DECONV1", "MVS_TRAIN_BN")
VALUES = (None, "", "0", "1", "hip", "taps", "torch", "miopen", "s1", "s2", "t2", "s1,t2", "s2,t2", "junk")
FEW = (None, "", "hip", "taps", "junk")   # the second and third switch of a routing grid
# (name, is_cuda, dtype, grad mode)
CONTEXTS = (("cuda,grad", True, torch.float32, True), ("cuda,no_grad", True, torch.float32, False),
            ("cpu,grad", False, torch.float32, True), ("cpu,no_grad", False, torch.float32, False),
            ("cuda,grad,f16", True, torch.float16, True))
ROUTE_CONTEXTS = CONTEXTS[:3]
LIVE_N = (20, 32, 40)   # a volume with live geometry (tests/test_bn_train_routing.py CHAIN_N)

S2_GRID = [(whole, splits, cin) for whole in (True, False)
           for splits in (None, (16, 32, 64), (16,), (32,), (64,), (16, 32)) for cin in (32, 16)]
S1_GRID = [(16, 16), (32, 32), (64, 64), (8, 8), (32, 16)]                       # weight (c_out, c_in)
T_GRID = [(no_dims, pair) for no_dims in (False, True) for pair in ((64, 32), (32, 16), (16, 8), (16, 16))]


class Stub:
    """What the predicates read of a tensor."""

    def __init__(self, is_cuda, dtype, shape):
        self.is_cuda, self.dtype, self.shape = is_cuda, dtype, tuple(shape)

    def dim(self):
        return len(self.shape)


def key(v):
    return "<unset>" if v is None else v


@contextlib.contextmanager
def environment(assignment):
    """Exactly ``assignment`` (None = unset) of the MVS_TRAIN_* variables, every other one unset."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("MVS_TRAIN_")}
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


def run_stack_parent():
    """The two reads of model._run_stack as the parent spelled them."""
    return [os.environ.get("MVS_TRAIN_CONV2D", "taps") == "taps", os.environ.get("MVS_TRAIN_CONV2D_FWD", "hip") == "hip"]


_FIXED = {}


def _fixed():
    if not _FIXED:
        from mvs_amd.config import pad_outpad
        from mvs_amd.model import CostVolumeReg
        pad, outpad = pad_outpad(*LIVE_N)
        _FIXED["reg"] = CostVolumeReg(pad=pad, outpad=outpad).train()
        _FIXED["conv"] = torch.nn.Conv3d(32, 8, 3, padding=1, bias=False)
    return _FIXED["reg"], _FIXED["conv"]


def predicates(is_cuda, dtype, run_stack=run_stack_parent):
    """{name: result} of every public predicate in the current environment and grad mode."""
    from mvs_amd import bn_train, model, narrow_train, region_train
    reg, conv = _fixed()
    x = Stub(is_cuda, dtype, (2, 32) + LIVE_N)
    out = {}
    for kind in (None, "s1", "s2", "t2"):
        out["region_train.enabled(%s)" % kind] = bool(region_train.enabled(x, kind))
    for kind in ("s1", "s2", "t2"):
        for c in (None, 16, 8):
            out["region_train.bwd_enabled(%s,%s)" % (kind, c)] = bool(region_train.bwd_enabled(kind, c))
    out["region_train.s2_bwd_enabled"] = bool(region_train.s2_bwd_enabled(x))
    out["region_train.t2_bwd_enabled"] = bool(region_train.t2_bwd_enabled(x))
    out["region_train.d1_enabled"] = bool(region_train.d1_enabled(x))
    for shape in ((16, 8), (32, 16)):
        out["region_train.d1_applies(%d,%d)" % shape] = bool(region_train.d1_applies(x, Stub(False, dtype, shape + (3, 3, 3))))
    out["bn_train.enabled"] = bool(bn_train.enabled(x))
    out["narrow_train.applies"] = bool(narrow_train.applies(conv, x))
    out["model.conv2d_bwd_mode"] = _outcome(model.conv2d_bwd_mode)
    out["CostVolumeReg.live_autograd_ok"] = bool(reg.live_autograd_ok(x))
    out["run_stack"] = _outcome(run_stack)
    return out


def _code(route):
    return "-" if route is None else str(2 * int(bool(route[0])) + int(bool(route[1])))


def s2_parent(x, w, whole, splits):
    """regions._conv_s2_region's condition, then region_train.s2_box's pair."""
    from mvs_amd import region_train as rt
    from mvs_amd.regions import _taps
    if not (_taps(x) and whole and splits is not None and x.shape[1] == 32
            and tuple(splits) in (rt.S2_SPLITS, (16,), (32,), (64,))
            and (rt.enabled(x, "s2") or rt.s2_bwd_enabled(x))):
        return None
    hip_bwd = rt.s2_bwd_enabled(x) and x.shape[1] == 32 and tuple(splits) == rt.S2_SPLITS
    return rt.enabled(x, "s2") or not rt.s2_bwd_enabled(x), hip_bwd


def s1_parent(x, w):
    """regions._conv_s1_region's condition, then _S1Valid.forward's backward kind (the forward is the HIP kernel)."""
    from mvs_amd import region_train as rt
    from mvs_amd.regions import _taps
    if not (_taps(x) and rt.enabled(x, "s1") and w.shape[0] == w.shape[1] and w.shape[0] in rt.S1_CHANNELS):
        return None
    return True, rt.bwd_enabled("s1", w.shape[0])


def tconv_parent(x, w, no_dims):
    """regions._tconv_region's two conditions, then t2_box's backward kind / d1_box (both directions on HIP)."""
    from mvs_amd import region_train as rt
    from mvs_amd.regions import _taps
    if not _taps(x):
        return None
    if not no_dims and rt.enabled(x, "t2") and (w.shape[0], w.shape[1]) in rt.T2_SHAPES:
        return True, rt.t2_bwd_enabled(x) and (w.shape[0], w.shape[1]) in rt.T2_SHAPES
    if no_dims and rt.d1_applies(x, w):
        return True, True
    return None


def route_rows(family, decide):
    """{key: one character per geometry of the family's grid} with ``decide`` = (s2, s1, tconv) functions."""
    rows = {}
    second = {"s2": "MVS_TRAIN_S2_BWD", "s1": "MVS_TRAIN_REGION_BWD", "tconv": "MVS_TRAIN_T2_BWD"}[family]
    for fwd in VALUES:
        for bwd in (VALUES if family != "tconv" else FEW):
            for d1 in (FEW if family == "tconv" else (None,)):
                env = {"MVS_TRAIN_REGION_FWD": fwd, second: bwd}
                if family == "tconv":
                    env["MVS_TRAIN_DECONV1"] = d1
                for name, is_cuda, dtype, grad in ROUTE_CONTEXTS:
                    with environment(env), torch.set_grad_enabled(grad):
                        if family == "s2":
                            row = [decide(Stub(is_cuda, dtype, (2, cin) + LIVE_N), None, whole, splits)
                                   for whole, splits, cin in S2_GRID]
                        elif family == "s1":
                            row = [decide(Stub(is_cuda, dtype, (2, ws[1], 9, 9, 9)), Stub(False, dtype, ws + (3, 3, 3)))
                                   for ws in S1_GRID]
                        else:
                            row = [decide(Stub(is_cuda, dtype, (2, pair[0], 5, 5, 5)),
                                          Stub(False, dtype, pair + (3, 3, 3)), no_dims) for no_dims, pair in T_GRID]
                    parts = [key(fwd), key(bwd)] + ([key(d1)] if family == "tconv" else []) + [name]
                    rows[";".join(parts)] = "".join(_code(r) for r in row)
    return rows


def predicate_table(run_stack=run_stack_parent):
    """(records, table): table[variable][value][context] indexes the list of distinct {predicate: result} records."""
    records, table = [], {}
    for var in VARIABLES:
        for v in VALUES:
            for name, is_cuda, dtype, grad in CONTEXTS:
                with environment({var: v}), torch.set_grad_enabled(grad):
                    rec = predicates(is_cuda, dtype, run_stack)
                if rec not in records:
                    records.append(rec)
                table.setdefault(var, {}).setdefault(key(v), {})[name] = records.index(rec)
    return records, table


if __name__ == "__main__":
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True).strip() \
        if os.path.isdir(os.path.join(REPO, ".git")) else os.environ.get("MVS_PINS_PARENT", "")
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    records, table = predicate_table()
    doc = {"parent": head, "records": records, "table": table,
           "routes": {"s2": route_rows("s2", s2_parent), "s1": route_rows("s1", s1_parent),
                      "tconv": route_rows("tconv", tconv_parent)}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d records, %d route rows (parent %s)"
          % (out, len(records), sum(len(v) for v in doc["routes"].values()), head))
