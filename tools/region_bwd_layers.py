"""Forward + backward time of the stride-1 region convolutions (conv_1_1 / conv_2_1 / conv_3_1 through
mvs_amd/region_train.py s1_valid) at the shapes of one cfg-2 train step, with the backward on the per-tap
GEMMs (MVS_TRAIN_REGION_BWD=taps, the default) against the HIP kernels (=s1): the calls of one step are
recorded, then each is timed alone, the two backends alternated --runs times; the HIP backward's two
kernels (input gradient on the region kernel, weight gradient on conv3d_region_wgrad) are also timed on
their own, the weight gradient with its useful-FLOP rate 2 * 27 * C^2 * output voxels / time.

Usage: python tools/region_bwd_layers.py [--reps N] [--runs N]   (prints one JSON line per layer)"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
import torch  # noqa: E402
from mvs_amd import ops, region_train  # noqa: E402

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
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    calls = []
    orig = region_train.s1_valid

    def rec(xin, w):
        calls.append((tuple(xin.shape), tuple(w.shape)))
        return orig(xin, w)
    region_train.s1_valid = rec
    net = bench.build_model(192, 512, 640, dev).train()
    img, K, R, T, d_min, d_int = bench.make_inputs(4, 3, 512, 640, 0, dev)
    ini, ref = net(img, K, R, T, d_min, d_int, 4, 3)
    (ini.sum() + ref.sum()).backward()
    region_train.s1_valid = orig
    del net, ini, ref
    torch.cuda.empty_cache()
    for xs, ws in calls:
        c = ws[0]
        x = torch.randn(xs, device=dev, requires_grad=True)
        w = (torch.randn(ws, device=dev) * 0.05).requires_grad_(True)
        gy = torch.randn((xs[0], c) + tuple(d - 2 for d in xs[2:]), device=dev)

        def fwd_bwd():
            x.grad = w.grad = None
            region_train.s1_valid(x, w).backward(gy)
        row = {"layer": "conv s1 C=%d" % c, "x": list(xs), "out_voxels": gy.numel() // c, "taps_ms": [], "hip_ms": []}
        for _ in range(a.runs):
            for key, val in (("taps_ms", "taps"), ("hip_ms", "s1")):
                os.environ["MVS_TRAIN_REGION_BWD"] = val
                row[key].append(round(timed(fwd_bwd, a.reps), 4))
        os.environ.pop("MVS_TRAIN_REGION_BWD")
        with torch.no_grad():
            x_cl = x.detach().permute(0, 2, 3, 4, 1).contiguous()
            gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
            wa = region_train._region_w_adjoint(w)
            L, out = list(xs[2:]), [d - 2 for d in xs[2:]]
            row["forward_ms"] = round(timed(lambda: region_train.s1_valid(x.detach(), w.detach()), a.reps), 4)
            row["hip_gw_ms"] = round(timed(lambda: ops.conv3d_region_wgrad(x_cl, gy_cl), a.reps), 4)
            row["hip_gx_ms"] = round(timed(lambda: ops.conv3d_region(gy_cl, None, wa, ops.CONV_S1, L, [0, 0, 0], L,
                                                                     [1, 1, 1], out, None, per_lane=True), a.reps), 4)
        tf = 2.0 * 27 * c * c * row["out_voxels"] / (row["hip_gw_ms"] * 1e-3) / 1e12
        row["hip_gw_TF"] = round(tf, 2)
        row["hip_gw_share_of_f32_matrix_peak"] = round(tf / PEAK_F32_MATRIX_TF, 4)
        print(json.dumps(row), flush=True)
        del x, w, gy, x_cl, gy_cl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
