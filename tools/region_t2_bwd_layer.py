"""Forward + backward time of the transposed region convolutions deconv_3_0 (64 -> 32) and deconv_2_0 (32 -> 16)
through mvs_amd/regions.py _tconv_region at the shapes of one cfg-2 train step (B = 4, the (192, 128, 160) volume,
the input on the M region of regions.live_regions, the output box the whole volume), with the backward on the
per-tap GEMMs (MVS_TRAIN_T2_BWD=taps, the default) against the HIP kernels (=hip), the forward on the HIP region
kernel both times; the two backends are alternated --runs times.  x and gy are given over channels-last memory,
the layout they reach _T2Box.backward in inside the train step.  The HIP backward's two kernels (weight gradient on
conv3d_t2_wgrad, input gradient on the region kernel's stride-2 mode) are also timed on their own, each with its
useful-FLOP rate 2 * 27 * c_in * c_out * B * input voxels / time against the f32 matrix peak (taps that land
outside the box are counted: an upper bound of a few percent), and the peak memory of one forward + backward is
recorded for both backends.

Usage: python tools/region_t2_bwd_layer.py [--reps N] [--runs N] [--batch B] [--dims D H W]   (one JSON line per
layer)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402,F401  (puts the package on the path)
import torch  # noqa: E402
from mvs_amd import ops, region_train, regions  # noqa: E402
from mvs_amd.config import pad_outpad  # noqa: E402

PEAK_F32_MATRIX_TF = 157.3


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


def _cl(shape, dev, rand):   # logical NCDHW over channels-last memory
    t = rand((shape[0],) + tuple(shape[2:]) + (shape[1],), device=dev)
    return t.permute(0, 4, 1, 2, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dims", type=int, nargs=3, default=[192, 128, 160])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = tuple(a.dims)
    pad, _ = pad_outpad(*n)
    full, M = regions.live_regions(n, pad)[:2]
    size = tuple(regions.extent(M))
    crop = tuple(lo - (2 * xlo - p) for (xlo, _), (lo, _), p in zip(M, full, pad))
    os.environ.pop("MVS_TRAIN_REGION_FWD", None)
    for name, (cin, cout) in zip(("deconv_3_0", "deconv_2_0"), region_train.T2_SHAPES):
        x = _cl((a.batch, cin) + size, dev, torch.rand).requires_grad_(True)
        w = (torch.randn(cin, cout, 3, 3, 3, device=dev) * 0.05).requires_grad_(True)
        gy = _cl((a.batch, cout) + n, dev, torch.randn)

        def fwd_bwd():
            x.grad = w.grad = None
            regions._tconv_region(x, M, w, full, pad, n).backward(gy)
        row = {"layer": "%s %d -> %d" % (name, cin, cout), "x": list(x.shape), "box": list(n), "crop": list(crop),
               "in_voxels": a.batch * size[0] * size[1] * size[2], "taps_ms": [], "hip_ms": []}
        for _ in range(a.runs):
            for key, val in (("taps_ms", "taps"), ("hip_ms", "hip")):
                os.environ["MVS_TRAIN_T2_BWD"] = val
                row[key].append(round(timed(fwd_bwd, a.reps), 4))
        for key, val in (("taps_peak_mem_GB", "taps"), ("hip_peak_mem_GB", "hip")):
            os.environ["MVS_TRAIN_T2_BWD"] = val
            x.grad = w.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            fwd_bwd()
            torch.cuda.synchronize()
            row[key] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
        os.environ.pop("MVS_TRAIN_T2_BWD")
        x.grad = w.grad = None
        torch.cuda.empty_cache()
        xd, wd = x.detach(), w.detach()
        # (grad mode on: _tconv_region takes the HIP region kernel only under autograd)
        row["forward_ms"] = round(timed(lambda: regions._tconv_region(xd, M, wd, full, pad, n), a.reps), 4)
        with torch.no_grad():
            row["hip_gw_ms"] = round(timed(lambda: ops.conv3d_t2_region_wgrad(xd, gy, crop), a.reps), 4)
            row["hip_gx_ms"] = round(timed(lambda: ops.conv3d_t2_region_dgrad(gy, wd, size, crop), a.reps), 4)
        flop = 2.0 * 27 * cin * cout * row["in_voxels"]
        for k in ("gw", "gx"):
            tf = flop / (row["hip_%s_ms" % k] * 1e-3) / 1e12
            row["hip_%s_TF" % k] = round(tf, 2)
            row["hip_%s_share_of_f32_matrix_peak" % k] = round(tf / PEAK_F32_MATRIX_TF, 4)
        print(json.dumps(row), flush=True)
        del x, w, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
