"""Device times of cloud evaluation (mvs_amd.cloud_eval) beside the same definition in chunked float64 torch ops on the
same device: profiles/cloud_eval_kernels.txt is this tool's output.

  python tools/cloud_eval_bench.py [--points 300000] [--rounds 5] [--iters 10] [--cells 0.5,1,2,4] [--out FILE]

Geometry: two synthetic sheets of DTU scale, 300 mm across with sub-millimetre spacing (300 mm / sqrt(points)), the
second 0.3 mm of noise away from the first; max_dist 20.  Per item a warm-up, then ``rounds`` alternations of
(feature x iters, torch baseline x 1), each timed with one event pair around the loop; the median per-call time over
the rounds and the min .. max spread are printed.  Items: the CloudIndex build, nearest on a built index,
evaluate_cloud (two builds, two searches, the reductions).  The baseline follows include/fusion/mvs_cloud_eval.h
pair by pair: chunk x G float64 d2, the gate, the minimum and its first index, as a user would write it without a
grid.  A sweep of explicit cell edges beside the default follows: the rule for the default was chosen from it."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "deep-multiview-depth-estimation_amd"))

from mvs_amd import cloud_eval  # noqa: E402

DEV = torch.device("cuda:0")
F64 = torch.float64
MAX_DIST = 20.0


def sheets(n, seed=0):
    rng = np.random.default_rng(seed)

    def one(noise):
        xy = rng.uniform(-150.0, 150.0, (n, 2))
        z = 25.0 * np.sin(xy[:, 0] / 60.0) + 0.1 * xy[:, 1] + rng.normal(0.0, noise, n)
        return torch.from_numpy((np.concatenate([xy, z[:, None]], 1) + [312.5, -187.25, 641.0]).astype(np.float32))
    return one(0.05).to(DEV), one(0.3).to(DEV)


def torch_nearest(query, target, max_dist, chunk_pairs=1 << 27):
    """(dist fp32, index int32) by the definition, float64, chunk x G pair distances at a time."""
    t = target.to(F64)
    t = t[torch.isfinite(t).all(1)]
    keep = torch.isfinite(target).all(1).nonzero()[:, 0]
    max2 = max_dist * max_dist
    chunk = max(1, chunk_pairs // max(len(t), 1))
    dist, index = [], []
    for a in range(0, len(query), chunk):
        q = query[a:a + chunk].to(F64)
        d = q[:, None, :] - t[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        d2 = torch.where(d2 <= max2, d2, torch.inf)
        best, j = d2.min(1)
        dist.append(torch.sqrt(best).to(torch.float32))
        index.append(torch.where(torch.isfinite(best), keep[j], -1).to(torch.int32))
    return torch.cat(dist), torch.cat(index)


def torch_evaluate(pred, gt, max_dist):
    a, b = torch_nearest(pred, gt, max_dist)[0], torch_nearest(gt, pred, max_dist)[0]
    return [float(d[torch.isfinite(d)].to(F64).mean()) for d in (a, b)]


def timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(name, ours, base, rounds, iters, log):
    ours()
    if base:
        base()
    t_ours, t_base = [], []
    for _ in range(rounds):
        t_ours.append(timed(ours, iters))
        if base:
            t_base.append(timed(base, 1))
    line = "%-34s %9.3f ms (%.3f .. %.3f)" % (name, statistics.median(t_ours), min(t_ours), max(t_ours))
    if base:
        line += "   torch float64 %10.1f ms (%.1f .. %.1f)   x%.0f" % (
            statistics.median(t_base), min(t_base), max(t_base), statistics.median(t_base) / statistics.median(t_ours))
    log(line)
    return statistics.median(t_ours)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cells", default="0.5,1,2,4,8")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    pred, gt = sheets(args.points)
    index = cloud_eval.CloudIndex(gt, MAX_DIST)
    log("two sheets of %d points, 300 mm across (spacing %.2f mm), max_dist %g; default cell %.3f mm, grid %s; "
        "median of %d rounds x %d calls (min .. max)" % (args.points, 300.0 / args.points ** 0.5, MAX_DIST,
                                                         index.cell, "x".join(map(str, index.dims)), args.rounds,
                                                         args.iters))
    ours, theirs = index.nearest(pred), (None if args.no_baseline else torch_nearest(pred, gt, MAX_DIST))
    if theirs is not None:
        same = torch.isinf(ours[0]) == torch.isinf(theirs[0])
        log("agreement with the baseline: found %s, max |dist| difference %.3g, index equal on %.6f of the queries"
            % (bool(same.all()), float((ours[0] - theirs[0]).nan_to_num(0.0, 0.0, 0.0).abs().max()),
               float((ours[1] == theirs[1]).double().mean())))
    base = None if args.no_baseline else (lambda: torch_nearest(pred, gt, MAX_DIST))
    compare("CloudIndex build", lambda: cloud_eval.CloudIndex(gt, MAX_DIST), None, args.rounds, args.iters, log)
    compare("nearest (pred -> gt)", lambda: index.nearest(pred), base, args.rounds, args.iters, log)
    compare("evaluate_cloud", lambda: cloud_eval.evaluate_cloud(pred, gt, MAX_DIST, (0.5, 1.0)),
            None if args.no_baseline else (lambda: torch_evaluate(pred, gt, MAX_DIST)), args.rounds, args.iters, log)
    log("cell sweep, nearest on a built index (points per occupied cell of a sheet = cell^2 points / 300^2):")
    for cell in [float(c) for c in args.cells.split(",") if c]:
        idx = cloud_eval.CloudIndex(gt, MAX_DIST, cell)
        compare("  cell %5.2f mm (%5.1f per cell)" % (cell, cell * cell * args.points / 9e4),
                lambda: idx.nearest(pred), None, args.rounds, args.iters, log)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
