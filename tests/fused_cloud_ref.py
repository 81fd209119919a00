"""The float64 restatement of the fused point cloud (include/fusion/mvs_view_fusion.h: mvs_fuse_views_fwd), in numpy,
fed the fp32 inputs widened, and the plane scenes of fusion_cases with a mask and colours, each restated once and
shared, unchanged, by test_fused_cloud_abi.py (the restatement's own conditions, no GPU) and test_fused_cloud_gpu.py.

There is no reference implementation: the rule in the header is the specification.  ``fuse`` follows it view by
view in index order and also returns ``taint``: the pixels whose outputs a rounding difference of 1e-14 relative
could change --
  * a slot decision within fusion_ref.NEAR of flipping (fusion_ref.consistency's own criteria),
  * xs + 0.5 or ys + 0.5 of a merged slot within NEAR of an integer (which pixel is absorbed),
  * a pixel whose ``used`` flag a tainted pixel could have set or not set: every pixel in the 3 x 3 block around
    where a tainted pixel lands in a later source view, for every non-empty slot, whatever the slot decided (a
    superset of what it could mark under either outcome; views go in index order, so one pass carries it forward)."""
import functools

import numpy as np

import fusion_cases
import fusion_ref

NEAR = fusion_ref.NEAR


def _blend(S, iy, ix, iy1, ix1, fx, fy):
    t = [S[a, b].astype(np.float64) for a, b in ((iy, ix), (iy, ix1), (iy1, ix), (iy1, ix1))]
    return (1.0 - fy) * ((1.0 - fx) * t[0] + fx * t[1]) + fy * ((1.0 - fx) * t[2] + fx * t[3])


def _slot(depth, colors, K, R, T, n, src, px_thresh, rel_thresh):
    """Steps 1-4 of mvs_geometric_consistency_fwd for every pixel of view n against source ``src``: (ok, near, xs, ys,
    d_r, [the source's colours blended at (xs, ys)] or None), as fusion_ref.consistency evaluates them."""
    N, _, h, w = depth.shape
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = depth[n, 0].astype(np.float64)
    M, m = fusion_ref.pair_matrix(K, R, T, n, src)
    Q, q = fusion_ref.pair_matrix(K, R, T, src, n)
    alive = d > 0
    nr = np.zeros((h, w), bool)
    # 1.
    zt = d * (M[2, 0] * x + M[2, 1] * y + M[2, 2])
    pz = zt + m[2]
    nr |= alive & (np.abs(pz) <= NEAR * (np.abs(zt) + abs(m[2])))
    alive = alive & (pz > 0)
    xs = (d * (M[0, 0] * x + M[0, 1] * y + M[0, 2]) + m[0]) / pz
    ys = (d * (M[1, 0] * x + M[1, 1] * y + M[1, 2]) + m[1]) / pz
    nr |= alive & ((np.abs(xs - np.rint(xs)) <= NEAR) | (np.abs(ys - np.rint(ys)) <= NEAR))
    # 2.
    x0, y0 = np.floor(xs), np.floor(ys)
    alive = alive & (x0 >= 0) & (x0 <= w - 2) & (y0 >= 0) & (y0 <= h - 2)
    ix = np.where(alive, x0, 0).astype(np.int64)
    iy = np.where(alive, y0, 0).astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
    S = depth[src, 0]
    alive = alive & (S[iy, ix] > 0) & (S[iy, ix1] > 0) & (S[iy1, ix] > 0) & (S[iy1, ix1] > 0)
    fx, fy = xs - x0, ys - y0
    ds = _blend(S, iy, ix, iy1, ix1, fx, fy)
    # 3.
    zt = ds * (Q[2, 0] * xs + Q[2, 1] * ys + Q[2, 2])
    qz = zt + q[2]
    nr |= alive & (np.abs(qz) <= NEAR * (np.abs(zt) + abs(q[2])))
    alive = alive & (qz > 0)
    xr = (ds * (Q[0, 0] * xs + Q[0, 1] * ys + Q[0, 2]) + q[0]) / qz
    yr = (ds * (Q[1, 0] * xs + Q[1, 1] * ys + Q[1, 2]) + q[1]) / qz
    # 4.
    lhs, px2 = (xr - x) ** 2 + (yr - y) ** 2, px_thresh * px_thresh
    nr |= alive & (np.abs(lhs - px2) <= NEAR * np.maximum(lhs, px2))
    gap, lim = np.abs(qz - d), rel_thresh * d
    nr |= alive & (np.abs(gap - lim) <= NEAR * np.maximum(gap, lim))
    ok = alive & (lhs < px2) & (gap < lim)
    col = None if colors is None else [_blend(colors[src, c], iy, ix, iy1, ix1, fx, fy) for c in range(3)]
    return ok, nr, xs, ys, qz, col


def fuse(depth, mask, colors, K, R, T, table, px_thresh=1.0, rel_thresh=0.01):
    """(emitted bool [N, h, w], n_merged int64 [N, h, w], xyz float64 [N, h, w, 3], rgb float64 [N, h, w, 3] or None,
    taint bool [N, h, w]) of depth fp32 [N, 1, h, w], mask [N, 1, h, w] (non-zero keeps), colors fp32 [N, 3, h, w] or
    None, fp32 cameras and the pair table [N, S]."""
    depth, mask, table = np.asarray(depth), np.asarray(mask), np.asarray(table)
    N, _, h, w = depth.shape
    Kd, Rd = np.asarray(K, np.float64), np.asarray(R, np.float64)
    Td = np.asarray(T, np.float64).reshape(-1, 3)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pix = np.stack([x, y, np.ones_like(x)], -1)
    used = np.zeros((N, h, w), bool)
    taint = np.zeros((N, h, w), bool)
    emitted = np.zeros((N, h, w), bool)
    merged = np.zeros((N, h, w), np.int64)
    xyz = np.zeros((N, h, w, 3))
    rgb = None if colors is None else np.zeros((N, h, w, 3))
    with np.errstate(all="ignore"):
        for n in range(N):
            d = depth[n, 0].astype(np.float64)
            cand = (mask[n, 0] != 0) & (d > 0)
            em = cand & ~used[n]
            total = np.zeros((h, w))
            cnt = np.zeros((h, w), np.int64)
            csum = None if colors is None else [colors[n, c].astype(np.float64) for c in range(3)]
            landings = []
            for s in range(table.shape[1]):
                src = int(table[n, s])
                if src < 0 or src >= N or src == n:
                    continue
                ok, nr, xs, ys, qz, col = _slot(depth, colors, K, R, T, n, src, px_thresh, rel_thresh)
                xh, yh = xs + 0.5, ys + 0.5
                nr = nr | (ok & ((np.abs(xh - np.rint(xh)) <= NEAR) | (np.abs(yh - np.rint(yh)) <= NEAR)))
                taint[n] |= nr & cand
                m = ok & em
                xn = np.clip(np.floor(xh[m]), 0, w - 1).astype(np.int64)
                yn = np.clip(np.floor(yh[m]), 0, h - 1).astype(np.int64)
                used[src, yn, xn] = True                 # (a mark on a view before n is never read)
                total = total + np.where(m, qz, 0.0)     # in slot order
                cnt = cnt + m
                if colors is not None:
                    csum = [a + np.where(m, b, 0.0) for a, b in zip(csum, col)]
                landings.append((src, xs, ys))
            # what a tainted pixel of this view could mark, under any outcome, in the views still to come
            t = taint[n] & cand
            if t.any():
                for src, xs, ys in landings:
                    sel = t & np.isfinite(xs) & np.isfinite(ys) & (np.abs(xs) < 2.0 ** 30) & (np.abs(ys) < 2.0 ** 30)
                    if src < n or not sel.any():
                        continue
                    cx, cy = np.rint(xs[sel]).astype(np.int64), np.rint(ys[sel]).astype(np.int64)
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            xx, yy = cx + dx, cy + dy
                            inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                            taint[src, yy[inside], xx[inside]] = True
            emitted[n] = em
            merged[n] = np.where(em, cnt, 0)
            dm = (d + total) / (1 + cnt)
            cam = dm[..., None] * (pix @ np.linalg.inv(Kd[n]).T) - Td[n]
            xyz[n] = np.where(em[..., None], cam @ Rd[n], 0.0)
            if colors is not None:
                rgb[n] = np.where(em[..., None], np.stack(csum, -1) / (1 + cnt)[..., None], 0.0)
    return emitted, merged, xyz, rgb, taint


def scene_colors(n_views, h, w):
    """[N, 3, h, w] fp32 in (0.1, 0.9): smooth, not constant along either axis, different per view and channel, so
    that a wrong tap, weight, channel or source view shows."""
    n, c, y, x = np.meshgrid(np.arange(n_views), np.arange(3), np.arange(h), np.arange(w), indexing="ij")
    v = 0.5 + 0.4 * np.sin(0.11 * x * (1.0 + 0.1 * c) + 0.07 * y * (1.0 + 0.05 * n) + 0.9 * n + 1.3 * c)
    return v.astype(np.float32)


def reversed_pairs(pairs, n_views):
    """The ragged pair list of the scene with its views in the opposite order."""
    return [[n_views - 1 - v if v >= 0 else v for v in row] for row in pairs[::-1]]


@functools.lru_cache(maxsize=None)
def fused_scene(h, w, n_views, n_slots):
    """fusion_cases.scene(...) with mask = (depth > 0) & (restated n_consistent >= 1) [N, 1, h, w] bool, colors, and
    the restatement's emitted, n_merged, xyz, rgb, taint (with colours: emitted, n_merged and xyz do not depend on
    them)."""
    sc = dict(fusion_cases.scene(h, w, n_views, n_slots))
    sc["mask"] = (sc["depth"] > 0) & (sc["count"] >= 1)
    sc["colors"] = scene_colors(n_views, h, w)
    out = fuse(sc["depth"], sc["mask"], sc["colors"], sc["K"], sc["R"], sc["T"], sc["table"])
    for key, a in zip(("emitted", "n_merged", "xyz", "rgb", "taint"), out):
        sc[key] = a
    for a in sc.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return sc
