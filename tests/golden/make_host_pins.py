"""Pins of the host layers (mvs_amd/ops.py wrappers, csrc/capi.hip weight splits): host_pins.json.

    python tests/golden/make_host_pins.py            # on a checkout + build of the PARENT commit

writes tests/golden/host_pins.json with the commit it ran on ("parent"); tests/test_host_refactor_pins.py
recomputes the same records with the code under test and compares.  The records:

  fragments  per weight-split entry point, weight shape and case: the SHA-256 of the fragment bytes and the
             returned exponent through the public ops.*_fragments functions; where those raise (the NaN
             case), the status the C entry point itself returns
  schemas    str(schema) of every registered mvs:: op
  fakes      (shape, dtype) of the fake kernels' outputs of the cost-volume family under FakeTensorMode

Weights are a closed-form integer hash scaled in float64 and cast to fp32: no RNG stream to drift.
No GPU is needed (the splits run on the host, the rest is metadata).
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(_HERE))
PINS = os.path.join(_HERE, "host_pins.json")
sys.path.insert(0, os.path.join(REPO, "deep-multiview-depth-estimation_amd"))

REGION_SHAPES = ((16, 16), (32, 32), (64, 64), (32, 64), (16, 32), (112, 32))   # (c_out, c_in); 112: train concat
CASES = ("hash", "zero", "pow2", "tiny", "huge", "nan")
GEOMETRY = (2, 3, 32, 16, 20, 12)   # (B, V, C, h, w, D) of the fake-kernel records


def hashed(n, seed):
    """n float64 values in [-0.5, 0.5) from a multiplicative integer hash of (index, seed)."""
    x = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed) * np.uint64(40503)) * np.uint64(2654435761)
    x &= np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return x.astype(np.float64) / 2.0 ** 32 - 0.5


def weight(shape, seed, case):
    """The fp32 weight of one case: hash values with max|w| set to 0.1-ish / 0 / 2^-1 / 1e-38 / 1e30, or one NaN."""
    n = int(np.prod(shape))
    v = hashed(n, seed)
    peak = seed % n                      # the element that carries the maximum
    unit = v / np.abs(v).max() * 0.999   # max|.| < 1, the peak element set below
    unit[peak] = 1.0
    if case == "hash":
        w = v * 0.2
    elif case == "zero":
        w = np.zeros(n)
    elif case == "pow2":
        w = unit * 0.5                   # max exactly 2^-1
    elif case == "tiny":
        w = unit * 1e-38                 # exponent rule clamps at +120
    elif case == "huge":
        w = unit * 1e30                  # negative exponent
    else:
        w = v * 0.2
        w[peak] = np.nan
    return torch.from_numpy(w.astype(np.float32).reshape(shape))


def fragment_targets():
    """(record key, ops function name, weight shape, C entry point, its integer arguments) of every
    weight-split entry point and model shape."""
    from mvs_amd import ops
    out = [("conv3d_split/8x32", "split_weight_fragments", (8, 32, 3, 3, 3), "mvs_conv3d_split_weights", ()),
           ("conv3d_s2_split/16x32", "_s2_split_fragments", (16, 32, 3, 3, 3), "mvs_conv3d_s2_split_weights", ())]
    for cin, cout, k, stride in sorted(ops.CONV2D_SPLIT_SHAPES):
        out.append(("conv2d_split/%dx%dk%d" % (cout, cin, k), "conv2d_split_fragments", (cout, cin, k, k),
                    "mvs_conv2d_split_weights", (cin, cout, k)))
    for cout, cin in REGION_SHAPES:
        out.append(("region_split/%dx%d" % (cout, cin), "region_split_fragments", (27, cout, cin),
                    "mvs_conv3d_region_split_weights", (cin, cout)))
    return out


def fragment_records():
    from mvs_amd import _lib, ops
    rec = {}
    for seed, (key, fn, shape, entry, ints) in enumerate(fragment_targets(), start=1):
        n = None
        for case in CASES:
            wt = weight(shape, seed, case)
            try:
                frag, e = getattr(ops, fn)(wt, torch.device("cpu"))
            except _lib.MVSLibraryError:   # the status behind the error, from the entry point itself
                out, ew = torch.zeros(n, dtype=torch.int16), ctypes.c_int(0)
                status = getattr(_lib.load(), entry)(_lib.ptr(wt), *ints, _lib.ptr(out), ctypes.byref(ew))
                rec["%s/%s" % (key, case)] = {"status": int(status)}
                continue
            assert frag.dtype == torch.int16 and n in (None, frag.numel())
            n = frag.numel()
            rec["%s/%s" % (key, case)] = {"status": 0, "exp": int(e), "n": frag.numel(),
                                          "sha256": hashlib.sha256(frag.numpy().tobytes()).hexdigest()}
    return rec


def schema_records():
    import mvs_amd  # noqa: F401  (registers the ops)
    names = sorted({n.split("::")[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names()
                    if n.startswith("mvs::")})
    return {n: str(getattr(torch.ops.mvs, n).default._schema) for n in names}


def fake_records():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from mvs_amd import ops
    B, V, C, h, w, D = GEOMETRY
    rec = {}

    def note(name, out):
        out = out if isinstance(out, (tuple, list)) else (out,)
        rec[name] = [[list(t.shape), str(t.dtype)] for t in out]

    with FakeTensorMode():
        feat, K, T = torch.empty(B * V, C, h, w), torch.empty(B * V, 3, 3), torch.empty(B * V, 3, 1)
        args = (feat, K, K, T, torch.empty(B), torch.empty(B), B, V, 0, D, 25.0)
        for name in ("cost_volume", "cost_volume_bf16", "cost_volume_c4", "cost_volume_c4_absmax",
                     "cost_volume_c4_split", "cost_volume_c4_bf16"):
            note(name, getattr(ops, name)(*args))
        w0, w1 = torch.empty(8, 32, 3, 3, 3), torch.empty(16, 32, 3, 3, 3)
        head = args + (w0, None, None, None, w1, None, None, None, [1, 1, 1], [0, 0, 0], [D // 2, h // 2, w // 2])
        note("cost_volume_head/boxed", ops.cost_volume_head(*head, [2, 0, 4], [D, h, w]))
        note("cost_volume_head/unboxed", ops.cost_volume_head(*head, [0, 0, 0], [0, 0, 0]))
    return rec


def records():
    return {"fragments": fragment_records(), "schemas": schema_records(), "fakes": fake_records()}


if __name__ == "__main__":
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True).strip()
    doc = {"parent": head}
    doc.update(records())
    with open(PINS, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d fragment records, %d schemas, %d fake records (parent %s)"
          % (PINS, len(doc["fragments"]), len(doc["schemas"]), len(doc["fakes"]), head))
