"""Float64 numpy restatement of the cloud-evaluation definition (include/fusion/mvs_cloud_eval.h), by
brute force over every pair, and the clouds the GPU tests run on.  No grid: the definition has none.

nearest() also flags the queries "near the gate": best within 1e-9 relative of max_dist^2, or a rejected candidate
within 1e-9 relative of it.  There a few units of 2^-53 (the kernel fuses the products of d2, numpy rounds each)
may decide whether a neighbour exists at all, so the GPU tests compare outside the flagged queries."""
import functools

import numpy as np

GATE_REL = 1e-9
SIZES = (1, 63, 64, 65, 1000, 5000)
MAX_DIST = 20.0
# DTU's world range: coordinates of hundreds of mm
OFFSET = np.array([312.5, -187.25, 641.0])


def nearest(query, target, max_dist, chunk=512):
    """(dist float64 [M] (+inf: none), index int64 [M] (-1: none), best d2 float64 [M] (+inf), flag bool [M]) for fp32
    arrays [M, 3] and [G, 3]; all arithmetic in float64 on the widened coordinates."""
    q, t = np.asarray(query, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    m, max2 = len(q), float(max_dist) * float(max_dist)
    best, index, flag = np.full(m, np.inf), np.full(m, -1, np.int64), np.zeros(m, bool)
    ok_t = np.isfinite(t).all(1)
    cand, orig = t[ok_t], np.flatnonzero(ok_t)
    if len(cand):
        for a in range(0, m, chunk):
            d = q[a:a + chunk, None, :] - cand[None, :, :]
            with np.errstate(invalid="ignore"):
                d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
                inside = d2 <= max2                                        # (a NaN fails it)
                gated = np.where(inside, d2, np.inf)
                near = np.abs(d2 - max2) <= GATE_REL * max2
            j = gated.argmin(1)                                            # (the first, so the lowest index, on a tie)
            b = gated[np.arange(len(j)), j]
            found = np.isfinite(b)
            best[a:a + chunk] = b
            index[a:a + chunk] = np.where(found, orig[j], -1)
            flag[a:a + chunk] = (near & ~inside).any(1) | (found & (np.abs(b - max2) <= GATE_REL * max2))
    bad_q = ~np.isfinite(q).all(1)
    best[bad_q], index[bad_q], flag[bad_q] = np.inf, -1, False
    return np.sqrt(best), index, best, flag


def pair_d2(query, target, i, j):
    """The restatement's d2 between query i and target j (arrays of indices), float64."""
    d = np.asarray(query, np.float32).astype(np.float64)[i] - np.asarray(target, np.float32).astype(np.float64)[j]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def evaluate(pred, gt, max_dist, thresholds=()):
    """evaluate_cloud's numbers from the restatement: float64 means of the fp32-rounded distances, the lower median,
    shares over the points with finite coordinates.  Also returns whether any query was flagged."""
    out, flagged = {}, False
    for name, short, a, b in (("accuracy", "pred", pred, gt), ("completeness", "gt", gt, pred)):
        dist, _, _, flag = nearest(a, b, max_dist)
        flagged |= bool(flag.any())
        d32 = dist.astype(np.float32)
        inl = np.sort(d32[np.isfinite(d32)].astype(np.float64))
        out[name] = float(inl.mean()) if len(inl) else float("nan")
        out[name + "_median"] = float(inl[(len(inl) - 1) // 2]) if len(inl) else float("nan")
        out["n_%s_inliers" % short] = len(inl)
        n_pts = int(np.isfinite(np.asarray(a, np.float32)).all(1).sum())
        out["precision" if short == "pred" else "recall"] = {
            float(tau): (float((d32.astype(np.float64) < float(tau)).sum()) / n_pts if n_pts else float("nan")) for tau in thresholds}
    out["overall"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["fscore"] = {}
    for tau in out["precision"]:
        p, r = out["precision"][tau], out["recall"][tau]
        out["fscore"][tau] = 0.0 if p == 0.0 and r == 0.0 else 2.0 * p * r / (p + r)
    return out, flagged


def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sheet(n, seed):
    """n points on a noisy sheet z = f(x, y) about 300 mm across (0.6 mm noise), offset to DTU's world range."""
    rng = np.random.default_rng(1000 + seed)
    xy = rng.uniform(-150.0, 150.0, (n, 2))
    z = 25.0 * np.sin(xy[:, 0] / 60.0) + 0.1 * xy[:, 1] + rng.normal(0.0, 0.6, n)
    return _frozen(np.concatenate([xy, z[:, None]], 1) + OFFSET)


@functools.lru_cache(maxsize=None)
def box(n, seed):
    """n points uniform in a 120 x 90 x 60 mm box, offset to DTU's world range."""
    rng = np.random.default_rng(2000 + seed)
    return _frozen(rng.uniform(-1.0, 1.0, (n, 3)) * np.array([60.0, 45.0, 30.0]) + OFFSET)


# (kind of the queries, M, kind of the targets, G): every size on either side, both kinds
CASES = tuple([("sheet", m, "sheet", g) for m, g in ((1, 5000), (63, 1000), (64, 65), (65, 64), (1000, 63),
                                                      (5000, 1), (5000, 5000), (1, 1))] +
              [("box", m, "box", g) for m, g in ((1000, 1000), (64, 5000), (5000, 63), (65, 65))] +
              [("box", 1000, "sheet", 5000), ("sheet", 5000, "box", 1000)])
MAKERS = {"sheet": sheet, "box": box}


def case_clouds(case):
    """(query, target) of a case; the two clouds come from different seeds."""
    qk, m, tk, g = case
    return MAKERS[qk](m, 1), MAKERS[tk](g, 2)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """nearest() of a case at MAX_DIST, computed once and shared (read-only arrays)."""
    out = nearest(*case_clouds(case), MAX_DIST)
    for a in out:
        a.setflags(write=False)
    return out
