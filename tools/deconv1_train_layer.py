"""Forward + backward time of deconv_1_0 (16 -> 8, the transposed region convolution whose output is the full-size
volume) through mvs_amd/regions.py _tconv_region at the shapes of one cfg-2 train step (B = 4, the input on the M
region of regions.live_regions, 97 x 65 x 81, the output box the whole (192, 128, 160) volume): the per-tap GEMMs
(MVS_TRAIN_DECONV1=taps, the default) against the HIP kernels (=hip: csrc/deconv3d_region.hip forward,
csrc/deconv3d_region_bwd.hip backward); the two are alternated --runs times.  x is given over channels-last memory
and gy NCDHW-contiguous, the layouts they reach _D1Box.backward in inside the train step.  The three
HIP kernels are also timed on their own, each with its time as a multiple of its one-pass HBM time: the bytes it
must move (forward: x in, y out; input gradient: gy in, gx out; weight gradient: gy and x in) over the measured
copy ceiling.  The peak memory of one forward + backward is recorded for both backends.

Usage: python tools/deconv1_train_layer.py [--reps N] [--runs N] [--batch B] [--dims D H W]   (one JSON line)"""
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

HBM_COPY_TBS = 6.29   # measured copy ceiling


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
    full, M = regions.live_regions(n, pad)[:2]
    size = tuple(regions.extent(M))
    crop = tuple(lo - (2 * xlo - p) for (xlo, _), (lo, _), p in zip(M, full, pad))
    cin, cout = region_train.D1_SHAPE
    x = torch.rand((a.batch,) + size + (cin,), device=dev).permute(0, 4, 1, 2, 3).requires_grad_(True)
    w = (torch.randn(cin, cout, 3, 3, 3, device=dev) * 0.05).requires_grad_(True)
    gy = torch.randn((a.batch, cout) + n, device=dev)

    def fwd_bwd():
        x.grad = w.grad = None
        regions._tconv_region(x, M, w, full, pad).backward(gy)
    in_vox, out_vox = a.batch * size[0] * size[1] * size[2], a.batch * n[0] * n[1] * n[2]
    row = {"layer": "deconv_1_0 %d -> %d" % (cin, cout), "x": list(x.shape), "box": list(n), "crop": list(crop),
           "in_voxels": in_vox, "taps_ms": [], "hip_ms": []}
    for _ in range(a.runs):
        for key, val in (("taps_ms", "taps"), ("hip_ms", "hip")):
            os.environ["MVS_TRAIN_DECONV1"] = val
            row[key].append(round(timed(fwd_bwd, a.reps), 4))
    for key, val in (("taps_peak_mem_GB", "taps"), ("hip_peak_mem_GB", "hip")):
        os.environ["MVS_TRAIN_DECONV1"] = val
        x.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fwd_bwd()
        torch.cuda.synchronize()
        row[key] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    os.environ.pop("MVS_TRAIN_DECONV1")
    x.grad = w.grad = None
    torch.cuda.empty_cache()
    xd, wd = x.detach(), w.detach()
    x_cl = xd.permute(0, 2, 3, 4, 1)
    with torch.no_grad():
        times = {"fwd": timed(lambda: ops.deconv3d_k3s2(x_cl, [0, 0, 0], wd, list(n), list(crop), None, None, None,
                                                        None, channels_last=True), a.reps),
                 "gw": timed(lambda: ops.deconv3d_k3s2_wgrad(xd, gy, crop), a.reps),
                 "gx": timed(lambda: ops.deconv3d_k3s2_dgrad(gy, wd, size, crop, channels_last=True), a.reps)}
    xb, yb = 4.0 * cin * in_vox, 4.0 * cout * out_vox
    for k, nbytes in (("fwd", xb + yb), ("gw", yb + xb), ("gx", yb + xb)):
        hbm_ms = nbytes / (HBM_COPY_TBS * 1e12) * 1e3
        row["hip_%s_ms" % k] = round(times[k], 4)
        row["hip_%s_MB" % k] = round(nbytes / 1e6, 1)
        row["hip_%s_one_pass_hbm_ms" % k] = round(hbm_ms, 4)
        row["hip_%s_x_hbm_time" % k] = round(times[k] / hbm_ms, 2)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
