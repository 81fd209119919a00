"""Forward + backward time of the twelve 2-D convolutions (eight encoder layers on 12 images of 512 x 640, four
refinement layers on 4 images of 128 x 160: one cfg-2 train step) each alone at its real input size, with the
backward on the per-tap GEMMs (MVS_TRAIN_CONV2D_BWD unset) against the HIP kernels (=hip), the two alternated
--runs times; the two HIP kernels are also timed on their own beside their one-pass HBM time (every operand read
or written once at 6.29 TB/s), and the layer's peak memory above its own tensors is reported for both.

Usage: python tools/conv2d_bwd_layers.py [--reps N] [--runs N]   (prints one JSON line per layer)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "deep-multiview-depth-estimation_amd"))
import torch  # noqa: E402
from mvs_amd import conv2d_train, model, tap_gemm  # noqa: E402

HBM_TBS = 6.29


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layers():
    """(name, (c_in, c_out, k, stride), (n, h, w)) of the twelve layers at cfg 2 (B 4, V 3, 512 x 640)."""
    out, h, w = [], 512, 640
    for i, (cin, cout, k, s, _) in enumerate(model._ENCODER):
        out.append(("encoder %d" % i, (cin, cout, k, s), (12, h, w)))
        h, w = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    for i, (cin, cout, k, s, _) in enumerate(model._REFINE):
        out.append(("refine %d" % i, (cin, cout, k, s), (4, 128, 160)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name, (cin, cout, k, s), (n, h, w) in layers():
        conv = torch.nn.Conv2d(cin, cout, k, stride=s, padding=k // 2, bias=False).to(dev)
        needs_gx = not name.startswith("encoder 0")   # the image needs no gradient
        x = torch.randn(n, cin, h, w, device=dev, requires_grad=needs_gx)
        with torch.no_grad():
            gy = torch.randn_like(tap_gemm.conv2d_hip_fwd(x, conv))

        def taps():
            x.grad = conv.weight.grad = None
            tap_gemm.conv2d_hip_fwd(x, conv).backward(gy)

        def hip():
            x.grad = conv.weight.grad = None
            conv2d_train.conv2d_hip(x, conv).backward(gy)
        row = {"layer": name, "shape": [cin, cout, k, s], "x": [n, cin, h, w], "needs_gx": needs_gx,
               "routed": (cin, cout, k, s) in conv2d_train.CONV2D_BWD_SHAPES, "taps_ms": [], "hip_ms": []}
        for _ in range(a.runs):
            for key, fn in (("taps_ms", taps), ("hip_ms", hip)):
                row[key].append(round(timed(fn, a.reps), 4))
        for key, fn in (("taps_peak_MB", taps), ("hip_peak_MB", hip)):
            x.grad = conv.weight.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            row[key] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
        with torch.no_grad():
            xd, wd = x.detach(), conv.weight.detach()
            row["forward_ms"] = round(timed(lambda: tap_gemm.conv2d_hip_fwd(xd, conv), a.reps), 4)
            row["hip_gw_ms"] = round(timed(lambda: conv2d_train.conv2d_wgrad(xd, gy, k, s), a.reps), 4)
            row["hip_gw_hbm_ms"] = round((xd.numel() + gy.numel()) * 4 / (HBM_TBS * 1e12) * 1e3, 4)
            if needs_gx:
                row["hip_gx_ms"] = round(timed(lambda: conv2d_train.conv2d_dgrad(gy, wd, s, h, w), a.reps), 4)
                row["hip_gx_hbm_ms"] = round((xd.numel() + gy.numel()) * 4 / (HBM_TBS * 1e12) * 1e3, 4)
        row["tiles_slots"] = list(conv2d_train.wgrad_plan(n, cin, cout, h, w, k, s))
        print(json.dumps(row), flush=True)
        del x, gy, conv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
