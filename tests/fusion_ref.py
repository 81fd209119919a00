"""Scenes and the float64 restatement for the depth-map filtering tests (test_fusion_abi.py, test_fusion_gpu.py).

There is no reference implementation of this step: the definitions in include/fusion/mvs_depth_filter.h are the
specification, and the functions here restate them step by step in numpy float64, fed the same fp32 inputs widened.

Scene: the world plane n . X = c seen by N cameras on an arc, all looking at one point of the plane; intrinsics
DTU-like and scaled to the map (fx = fy = 361.54 w / 160, the principal point near the centre and off the pixel
grid); each view's depth map is the exact ray-plane depth in float64 rounded to fp32; distances 425-935."""
import numpy as np

PLANE_N = np.array([0.12, -0.07, 1.0]) / np.linalg.norm([0.12, -0.07, 1.0])
PLANE_C = 0.0
NEAR = 1e-9


def arc_cameras(n_views, h, w, radius=640.0, spread=0.05, growth=0.013):
    """K, R [N, 3, 3], T [N, 3, 1] fp32: cameras on an arc about the origin (a point of the plane), ``spread``
    radians apart at distances radius (1 + growth i), each looking at the origin; x_cam = R x_world + T."""
    Ks, Rs, Ts = [], [], []
    for i in range(n_views):
        a = spread * (i - 0.5 * (n_views - 1)) + 0.013
        C = radius * np.array([np.sin(a), 0.021 * (i % 3) - 0.017, -np.cos(a)]) * (1.0 + growth * i)
        rz = -C / np.linalg.norm(C)
        rx = np.cross(np.array([0.0, 1.0, 0.0]), rz)
        rx /= np.linalg.norm(rx)
        ry = np.cross(rz, rx)
        R = np.stack([rx, ry, rz])
        f = 361.54 * w / 160.0
        K = np.array([[f, 0.0, 0.5 * (w - 1) + 0.137 + 0.031 * i], [0.0, f, 0.5 * (h - 1) - 0.211 + 0.017 * i],
                      [0.0, 0.0, 1.0]])
        Ks.append(K)
        Rs.append(R)
        Ts.append((-R @ C).reshape(3, 1))
    f32 = lambda a: np.stack(a).astype(np.float32)
    return f32(Ks), f32(Rs), f32(Ts)


def plane_depths(K, R, T, h, w):
    """[N, 1, h, w] fp32: each (fp32) camera's exact z-depth of the plane, float64 rounded once."""
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], 0).reshape(3, -1)
    out = []
    for Kn, Rn, Tn in zip(K.astype(np.float64), R.astype(np.float64), T.astype(np.float64)):
        C = -Rn.T @ Tn.reshape(3)
        ray = Rn.T @ (np.linalg.inv(Kn) @ pix)               # world direction per unit camera depth
        d = (PLANE_C - PLANE_N @ C) / (PLANE_N @ ray)
        out.append(d.reshape(1, h, w))
    d = np.stack(out)
    assert d.min() > 425.0 and d.max() < 935.0, (d.min(), d.max())
    return d.astype(np.float32)


def pad_pairs(pairs):
    """A ragged nested list as an int array [N, S], -1 padded, S >= 1."""
    width = max([len(r) for r in pairs] + [1])
    return np.array([list(r) + [-1] * (width - len(r)) for r in pairs], dtype=np.int64).reshape(len(pairs), width)


def pair_matrix(K, R, T, a, b):
    """(M, m) of camera a -> camera b, float64: M = K_b R_b R_a^T K_a^-1, m = K_b (T_b - R_b R_a^T T_a)."""
    K, R, T = (np.asarray(t, np.float64) for t in (K, R, T))
    T = T.reshape(-1, 3)
    M = (K[b] @ R[b]) @ (R[a].T @ np.linalg.inv(K[a]))
    m = K[b] @ (T[b] - (R[b] @ R[a].T) @ T[a])
    return M, m


def non_empty_slots(table):
    table = np.asarray(table)
    n = table.shape[0]
    return np.array([sum(1 for v in table[i] if 0 <= v < n and v != i) for i in range(n)])


def consistency(depth, K, R, T, table, px_thresh=1.0, rel_thresh=0.01):
    """The restatement of mvs_geometric_consistency_fwd: (n_consistent int64 [N, 1, h, w], depth_avg float64
    [N, 1, h, w], near bool [N, 1, h, w]).  ``near``: a pixel some decision of which is within NEAR of flipping --
    xs or ys within 1e-9 of an integer, p.z or q.z within 1e-9 of the magnitude of its terms from 0, either side of
    a threshold comparison within 1e-9 relative of the other."""
    depth = np.asarray(depth)
    table = np.asarray(table)
    N, _, h, w = depth.shape
    ys, xs_ = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    count = np.zeros((N, 1, h, w), np.int64)
    avg = np.zeros((N, 1, h, w), np.float64)
    near = np.zeros((N, 1, h, w), bool)
    with np.errstate(all="ignore"):
        for n in range(N):
            d = depth[n, 0].astype(np.float64)
            valid = d > 0
            total = np.zeros((h, w))
            cnt = np.zeros((h, w), np.int64)
            nr = np.zeros((h, w), bool)
            for s in range(table.shape[1]):
                src = int(table[n, s])
                if src < 0 or src >= N or src == n:
                    continue
                M, m = pair_matrix(K, R, T, n, src)
                Q, q = pair_matrix(K, R, T, src, n)
                x, y = xs_, ys
                # 1.
                zt = d * (M[2, 0] * x + M[2, 1] * y + M[2, 2])
                pz = zt + m[2]
                alive = valid.copy()
                nr |= alive & (np.abs(pz) <= NEAR * (np.abs(zt) + abs(m[2])))
                alive &= pz > 0
                xs = (d * (M[0, 0] * x + M[0, 1] * y + M[0, 2]) + m[0]) / pz
                ysrc = (d * (M[1, 0] * x + M[1, 1] * y + M[1, 2]) + m[1]) / pz
                nr |= alive & ((np.abs(xs - np.rint(xs)) <= NEAR) | (np.abs(ysrc - np.rint(ysrc)) <= NEAR))
                # 2.
                x0, y0 = np.floor(xs), np.floor(ysrc)
                alive &= (x0 >= 0) & (x0 <= w - 2) & (y0 >= 0) & (y0 <= h - 2)
                ix = np.where(alive, x0, 0).astype(np.int64)
                iy = np.where(alive, y0, 0).astype(np.int64)
                S = depth[src, 0]
                ix1, iy1 = np.minimum(ix + 1, w - 1), np.minimum(iy + 1, h - 1)
                t00, t01, t10, t11 = S[iy, ix], S[iy, ix1], S[iy1, ix], S[iy1, ix1]
                alive &= (t00 > 0) & (t01 > 0) & (t10 > 0) & (t11 > 0)
                fx, fy = xs - x0, ysrc - y0
                t00, t01, t10, t11 = (t.astype(np.float64) for t in (t00, t01, t10, t11))
                ds = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t01) + fy * ((1.0 - fx) * t10 + fx * t11)
                # 3.
                zt = ds * (Q[2, 0] * xs + Q[2, 1] * ysrc + Q[2, 2])
                qz = zt + q[2]
                nr |= alive & (np.abs(qz) <= NEAR * (np.abs(zt) + abs(q[2])))
                alive &= qz > 0
                xr = (ds * (Q[0, 0] * xs + Q[0, 1] * ysrc + Q[0, 2]) + q[0]) / qz
                yr = (ds * (Q[1, 0] * xs + Q[1, 1] * ysrc + Q[1, 2]) + q[1]) / qz
                # 4.
                lhs = (xr - x) ** 2 + (yr - y) ** 2
                px2 = px_thresh * px_thresh
                nr |= alive & (np.abs(lhs - px2) <= NEAR * np.maximum(lhs, px2))
                gap, lim = np.abs(qz - d), rel_thresh * d
                nr |= alive & (np.abs(gap - lim) <= NEAR * np.maximum(gap, lim))
                ok = alive & (lhs < px2) & (gap < lim)
                total = total + np.where(ok, qz, 0.0)
                cnt = cnt + ok
            count[n, 0] = np.where(valid, cnt, 0)
            avg[n, 0] = np.where(valid, (d + total) / (1 + cnt), 0.0)
            near[n, 0] = nr
    return count, avg, near


def confidence(prob, depth, d_batch):
    """The restatement of mvs_photometric_confidence_fwd in float64: (conf [B, 1, h, w], t [B, 1, h, w])."""
    prob, depth = np.asarray(prob, np.float64), np.asarray(depth, np.float64)
    B, _, D, h, w = prob.shape
    db = np.asarray(d_batch, np.float64).reshape(-1, D)
    if db.shape[0] == 1:
        db = np.repeat(db, B, 0)
    with np.errstate(all="ignore"):
        t = (depth - db[:, 0].reshape(B, 1, 1, 1)) / (db[:, 1] - db[:, 0]).reshape(B, 1, 1, 1)
        k0 = np.clip(np.floor(np.where(np.isnan(t), 0.0, t)), 0, D - 1).astype(np.int64)
    conf = np.zeros((B, 1, h, w))
    for k in range(-1, 3):
        kk = k0 + k
        inside = (kk >= 0) & (kk < D)
        conf = conf + np.where(inside, np.take_along_axis(prob[:, 0], np.clip(kk, 0, D - 1), 1), 0.0)
    return np.where(np.isnan(t), 0.0, conf), t


def backproject(depth, K, R, T):
    """The restatement of mvs_backproject_fwd in float64: xyz [N, h, w, 3]."""
    depth = np.asarray(depth)
    N, _, h, w = depth.shape
    K, R, T = (np.asarray(t, np.float64) for t in (K, R, T))
    T = T.reshape(-1, 3)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pix = np.stack([xs, ys, np.ones_like(xs)], -1)                      # [h, w, 3]
    out = np.zeros((N, h, w, 3))
    for n in range(N):
        d = depth[n, 0].astype(np.float64)
        cam = d[..., None] * (pix @ np.linalg.inv(K[n]).T) - T[n]
        out[n] = np.where((d > 0)[..., None], cam @ R[n], 0.0)           # R^T cam, row-wise
    return out
