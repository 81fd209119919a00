"""Forward + backward time of one train-mode BatchNorm + ReLU site of CostVolumeReg.forward_live_train at the shapes
of a cfg-2 train step (B = 4, volume (192, 128, 160)): the torch passes (bn_sums._sums / _bn_train / _apply_bn / ReLU
and regions._crop_pad, what MVS_TRAIN_BN=torch runs) against the fused node (bn_train.bn_relu_train, =hip), the two
alternated --runs times.  Sites: `y0` (conv_0_0's output, 8 channels, NCDHW, no box: 503 MB) and `deconv_3_0`'s
output (32 channels, channels-last memory, the box M: 2.0 GB).  Each time is set against the HBM time of five passes
over the tensor (forward: read for the sums, read + write for the BN; backward: two reads of z, one write of gz; gy
and the output on a box M are an eighth of it and not counted) at the measured copy ceiling.  The peak memory of one
forward + backward is recorded for both.

Usage: python tools/bn_train_site.py [--reps N] [--runs N] [--batch B] [--dims D H W]   (one JSON line per site)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402,F401  (puts the package on the path)
import torch  # noqa: E402
from mvs_amd import bn_train, regions  # noqa: E402
from mvs_amd.bn_sums import _apply_bn, _bn_train, _sums  # noqa: E402
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
    count = a.batch * n[0] * n[1] * n[2]
    for name, c, cl, box in (("y0", 8, False, None), ("deconv_3_0 output", 32, True, M)):
        bn = torch.nn.BatchNorm3d(c, device=dev).train()
        z = torch.randn((a.batch,) + n + (c,) if cl else (a.batch, c) + n, device=dev)
        z = (z.permute(0, 4, 1, 2, 3) if cl else z).requires_grad_(True)
        gy = torch.randn((a.batch, c) + tuple(regions.extent(box if box is not None else full)), device=dev)

        def torch_site():
            z.grad = bn.weight.grad = bn.bias.grad = None
            p = _bn_train(bn, *_sums(z), count)
            y = torch.relu(_apply_bn(z if box is None else regions._crop_pad(z, full, box, n), *p))
            y.backward(gy)

        def hip_site():
            z.grad = bn.weight.grad = bn.bias.grad = None
            bn_train.bn_relu_train(z, box, bn, None, count)[0].backward(gy)
        nbytes = 4.0 * z.numel()
        row = {"site": name, "z": list(z.shape), "channels_last": cl, "box": None if box is None else list(box),
               "MB": round(nbytes / 1e6, 1), "torch_ms": [], "hip_ms": []}
        for _ in range(a.runs):
            row["torch_ms"].append(round(timed(torch_site, a.reps), 4))
            row["hip_ms"].append(round(timed(hip_site, a.reps), 4))
        for key, fn in (("torch_peak_mem_GB", torch_site), ("hip_peak_mem_GB", hip_site)):
            z.grad = bn.weight.grad = bn.bias.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            row[key] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
        row["five_pass_hbm_ms"] = round(5.0 * nbytes / (HBM_COPY_TBS * 1e12) * 1e3, 4)
        row["hip_x_five_pass_hbm_time"] = round(min(row["hip_ms"]) / row["five_pass_hbm_ms"], 2)
        row["torch_x_five_pass_hbm_time"] = round(min(row["torch_ms"]) / row["five_pass_hbm_ms"], 2)
        print(json.dumps(row), flush=True)
        del z, gy, bn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
