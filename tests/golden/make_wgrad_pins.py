"""Bit pins of the tap-row weight-gradient kernels (csrc/conv3d_region_wgrad.hip, csrc/conv3d_s2_wgrad.hip,
csrc/conv3d_t2_wgrad.hip and the weight-gradient half of csrc/deconv3d_region_bwd.hip): wgrad_pins.json.

    python tests/golden/make_wgrad_pins.py          # on a checkout + build of the PARENT commit, on the GPU

writes tests/golden/wgrad_pins.json with the commit it ran on ("parent"); tests/test_wgrad_pins.py recomputes the
same records through the mvs_amd.ops wrappers with the code under test and compares.  Per case the record is the
SHA-256 of dw's bytes.

The kernels sum their partial slots in slot order without atomics, so the hashes are run-to-run stable: the
generator runs every case twice and compares before it writes.  Inputs come from a CPU torch.Generator seeded by
the case's name.

One case per kernel instantiation -- stride 1 C = 16 / 32 / 64, stride 2 32 -> 112, transposed (64, 32) and
(32, 16), deconv_1_0 with x channels-last and NCDHW -- each at two shapes:
  single  one pass of the tile loop; no extent a multiple of 16 and the row count no multiple of any TR, so the
          last x tile and the last row tile are partly filled; pad_lo / crop non-zero, so tap rows fall off the
          volume / the box (skipped rows).
            stride 1: B = 2, crop (9, 9, 23): outputs (7, 7, 21), 98 rows (98 mod 28 / 10 / 6 = 14 / 8 / 2)
            stride 2: B = 2, volume (11, 9, 37), pad_lo (1, 1, 1), box (6, 4, 19): 48 rows (mod 5 = 3); the last
                      outputs along z and x read one past the volume
            transposed and deconv_1_0: B = 2, x (4, 5, 21), crop (1, 2, 5), box (5, 6, 35): 40 rows
                      (mod 6 / 12 / 16 = 4 / 4 / 8); test_region_train_t2_bwd.py's second geometry
  multi   the smallest shape the multi-pass tests use for the instantiation (tiles > 2 x 168, ragged last pass):
          test_region_train_multipass.py S1_CASES and S2_GEO, test_region_train_t2_bwd.py MULTI,
          test_deconv1_train.py MULTI (534 tiles).
"""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(_HERE))
PINS = os.path.join(_HERE, "wgrad_pins.json")
_PKG = os.path.join(REPO, "deep-multiview-depth-estimation_amd")
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

S1_SINGLE = (2, (9, 9, 23))
S1_MULTI = {64: (3, (20, 19, 52)), 32: (3, (20, 19, 52)), 16: (2, (42, 42, 38))}
S2_SINGLE = (2, (11, 9, 37), (1, 1, 1), (6, 4, 19))
S2_MULTI = (3, (27, 28, 79), (1, 0, 1), (14, 14, 40))
T_SINGLE = (2, (4, 5, 21), (1, 2, 5), (5, 6, 35))
T2_MULTI = {(64, 32): (3, (16, 15, 40), (1, 0, 1), (31, 31, 82)),
            (32, 16): (3, (24, 20, 40), (1, 0, 1), (47, 41, 82))}
D1_MULTI = (3, (21, 45, 40), (1, 0, 1), (41, 89, 82))


def cases():
    """{key: (runner name, arguments)} of every pinned case (no GPU, no torch op needed)."""
    out = {}
    for c in (16, 32, 64):
        out["s1_%d/single" % c] = ("s1", (c,) + S1_SINGLE)
        out["s1_%d/multi" % c] = ("s1", (c,) + S1_MULTI[c])
    out["s2_32_112/single"] = ("s2", S2_SINGLE)
    out["s2_32_112/multi"] = ("s2", S2_MULTI)
    for pair in ((64, 32), (32, 16)):
        out["t2_%d_%d/single" % pair] = ("t2", (pair,) + T_SINGLE)
        out["t2_%d_%d/multi" % pair] = ("t2", (pair,) + T2_MULTI[pair])
    for layout in ("channels_last", "ncdhw"):
        out["d1_%s/single" % layout] = ("d1", (layout,) + T_SINGLE)
        out["d1_%s/multi" % layout] = ("d1", (layout,) + D1_MULTI)
    return out


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def _as_cl(t):
    """A logical NCDHW tensor over channels-last memory."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def _run_s1(g, dev, c, b, L):
    from mvs_amd import ops
    x = torch.randn((b,) + L + (c,), generator=g).to(dev)
    gy = torch.randn((b,) + tuple(d - 2 for d in L) + (c,), generator=g).to(dev)
    return ops.conv3d_region_wgrad(x, gy)


def _run_s2(g, dev, b, dims, pad_lo, out):
    from mvs_amd import ops
    x = torch.randn((b, 32) + dims, generator=g).to(dev)
    gy = torch.randn((b,) + out + (112,), generator=g).to(dev)
    return ops.conv3d_s2_region_wgrad(x, gy, pad_lo)


def _run_t2(g, dev, pair, b, size, crop, out):
    from mvs_amd import ops
    x = torch.randn((b, pair[0]) + size, generator=g).to(dev)
    gy = torch.randn((b, pair[1]) + out, generator=g).to(dev)
    return ops.conv3d_t2_region_wgrad(_as_cl(x), _as_cl(gy), crop)


def _run_d1(g, dev, layout, b, size, crop, out):
    from mvs_amd import ops
    x = torch.randn((b, 16) + size, generator=g).to(dev)
    gy = torch.randn((b, 8) + out, generator=g).to(dev)
    return ops.deconv3d_k3s2_wgrad(_as_cl(x) if layout == "channels_last" else x, gy, crop)


_RUNNERS = {"s1": _run_s1, "s2": _run_s2, "t2": _run_t2, "d1": _run_d1}


def run_case(key):
    """The record of one case on cuda:0."""
    runner, args = cases()[key]
    dw = _RUNNERS[runner](_gen(key), torch.device("cuda", 0), *args)
    torch.cuda.synchronize()
    # no pin of a degenerate result: every tap of every channel pair has terms at these shapes
    assert torch.isfinite(dw).all().item() and bool((dw != 0).all()), "degenerate dw: %s" % key
    return {"dw": _sha(dw)}


if __name__ == "__main__":
    head = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=REPO, text=True).strip() \
        if os.path.isdir(os.path.join(REPO, ".git")) else os.environ.get("MVS_PINS_PARENT", "")
    out = sys.argv[1] if len(sys.argv) > 1 else PINS
    doc = {"parent": head, "cases": {}}
    for key in sorted(cases()):
        first = run_case(key)
        again = run_case(key)
        assert first == again, "not run-to-run stable: %s" % key
        doc["cases"][key] = first
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases (parent %s)" % (out, len(doc["cases"]), head))
