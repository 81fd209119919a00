"""Forward + backward time of the stacked stride-2 region convolution (conv_1_0 / conv_2_0 / conv_3_0 as one
32 -> 112 layer through mvs_amd/regions.py _conv_s2_region) at the shapes of one cfg-2 train step (B = 4, the
(192, 128, 160) cost volume, the output box R2 of regions.live_regions), with the backward on the per-tap GEMMs
(MVS_TRAIN_S2_BWD=taps, the default) against the HIP kernels (=hip), the forward on the tap GEMMs both times;
the two backends are alternated --runs times.  The HIP backward's two kernels (weight gradient on
conv3d_s2_wgrad, input gradient on the region kernel's transposed mode) are also timed on their own, each with
its useful-FLOP rate 2 * 27 * 32 * 112 * B * output voxels / time against the f32 matrix peak, and the peak
memory of one forward + backward is recorded for both backends.

Usage: python tools/region_s2_bwd_layer.py [--reps N] [--runs N] [--batch B] [--dims D H W]   (one JSON line)"""
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
    M = regions.live_regions(n, pad)[1]
    R2 = regions._grow(M, n, 2)
    size = tuple(regions.extent(R2))
    pl = tuple(max(2 * lo - p, 0) - (2 * lo - p) for (lo, _), p in zip(R2, pad))
    x = torch.rand((a.batch, 32) + n, device=dev, requires_grad=True)
    w = (torch.randn(112, 32, 3, 3, 3, device=dev) * 0.05).requires_grad_(True)
    gy = torch.randn((a.batch, 112) + size, device=dev)
    os.environ.pop("MVS_TRAIN_REGION_FWD", None)

    def fwd_bwd():
        x.grad = w.grad = None
        regions._conv_s2_region(x, w, R2, pad, splits=region_train.S2_SPLITS).backward(gy)
    row = {"layer": "conv s2 32 -> 16 + 32 + 64", "x": list(x.shape), "box": list(size), "pad_lo": list(pl),
           "out_voxels": a.batch * size[0] * size[1] * size[2], "taps_ms": [], "hip_ms": []}
    for _ in range(a.runs):
        for key, val in (("taps_ms", "taps"), ("hip_ms", "hip")):
            os.environ["MVS_TRAIN_S2_BWD"] = val
            row[key].append(round(timed(fwd_bwd, a.reps), 4))
    for key, val in (("taps_peak_mem_GB", "taps"), ("hip_peak_mem_GB", "hip")):
        os.environ["MVS_TRAIN_S2_BWD"] = val
        x.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd()
        torch.cuda.synchronize()
        row[key] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    os.environ.pop("MVS_TRAIN_S2_BWD")
    x.grad = w.grad = None
    torch.cuda.empty_cache()
    with torch.no_grad():
        gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
        xd, wd = x.detach(), w.detach()
        row["forward_ms"] = round(timed(lambda: regions._conv_s2_region(xd, wd, R2, pad,
                                                                       splits=region_train.S2_SPLITS), a.reps), 4)
        row["hip_gw_ms"] = round(timed(lambda: ops.conv3d_s2_region_wgrad(xd, gy_cl, pl), a.reps), 4)
        row["hip_gx_ms"] = round(timed(lambda: ops.conv3d_s2_region_dgrad(gy_cl, wd, n, pl), a.reps), 4)
    flop = 2.0 * 27 * 32 * 112 * row["out_voxels"]
    for k in ("gw", "gx"):
        tf = flop / (row["hip_%s_ms" % k] * 1e-3) / 1e12
        row["hip_%s_TF" % k] = round(tf, 2)
        row["hip_%s_share_of_f32_matrix_peak" % k] = round(tf / PEAK_F32_MATRIX_TF, 4)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
