"""Synthetic camera rigs beyond the DTU geometry, and the references that go with them (test helper).

Every cost-volume test before tests/test_camera_geometry.py took its cameras from
tests/golden/cameras.py (the DTU scan-1 rigs: neighbouring views a few degrees apart, the
homogeneous coordinate s positive everywhere, footprints of about 36 x 10 per 32 x 8 tile).  The
families below are valid cameras that reach the rest of the kernels' code: samples behind the source
camera (s < 0), poles inside a tile, |s| <= 1e-8 (kornia's undivided rule), a singular homography,
a view that sees nothing, tall footprints, and footprints whose sum exceeds the backward's LDS.

Layouts are those of ``cameras.camera_batch`` / ``depth_range``: K, R [B*V, 3, 3], T [B*V, 3, 1],
d_min, d_int [B, 1, 1, 1], all fp32.  Per sample, view 0 is the reference camera (R = I, centre at
the origin, K = [[f, 0, (w-1)/2], [0, f, (h-1)/2], [0, 0, 1]]); source view i has rotation R_i and
centre C_i (T_i = -R_i C_i).  Depth planes are d_min + 25 d_int k with d_min = 425, d_int = 1 in
every family, so the view-major depth tiling of homography.py:24-26 (image i uses sample i mod B)
cannot mix two families' planes.

The sampling map of the reference project is inv(H) applied to the reference pixel (kornia's
warp_perspective inverts the matrix it is given), H = K_i R_i (I - C_i n^T / d) K_r^-1.  With
y = R_i^T K_i^-1 [x, y, 1] the homogeneous coordinate is s = y_z d / (d - C_i,z): negative where
the pixel's ray, taken as a ray of the source camera, points backwards (y_z < 0) or where the
source centre lies beyond the plane (C_z > d); H is singular where C_z = d.

numpy and torch only; nothing from the reference project.
"""
import numpy as np
import torch

from test_sampling_law import fma32, norm_coord, sample_coord, sample_law

f32 = np.float32
D_MIN, D_INT, D_SCALE = 425.0, 1.0, 25.0
TILE_W, TILE_H = 32, 8          # the forward's and the backward's pixel tile
BWD_SLOTS = 49152 // (8 * 5)    # cost_volume_bwd.hip: bwd_slots()
BWD_PLANES = 32                 # cost_volume_bwd.hip: kBwdKPG

FAMILIES = ("roll", "pole", "behind", "quarter_turn", "singular", "blind")
SHAPES = ((20, 36), (37, 53), (64, 80))
ZOOM_SHAPE = (128, 160)
ZOOM_SCALES = (0.2, 0.2, 0.25, 0.25, 0.3, 4.0, 8.0)


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _quarter(k):
    """Rotation by k quarter turns about the optical axis, exact entries."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


_QT = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)


def _sources(family, w):
    """(focal length / w, [(R_i, C_i)] of the family's own source views, the centre step that
    separates a cycled copy of a view from the view itself)."""
    deg = np.pi / 180
    if family == "roll":
        return 1.2, [(_quarter(1), (15.0, 4.0, 0.0)), (_quarter(2), (-3.0, 17.0, 0.0)),
                     (_quarter(3), (-20.0, -2.0, 0.0))], (6.0, -5.0, 3.0)
    if family == "pole":
        return 0.35, [(rot_y(50 * deg), (30.0, 0.0, 0.0)),
                      (rot_z(0.3) @ rot_y(-55 * deg), (-21.0, 21.0, 4.0))], (5.0, 7.0, -6.0)
    if family == "behind":
        return 1.2, [(np.eye(3), (5.0, 0.0, 460.0)), (np.eye(3), (0.0, 4.0, 900.0))], (3.0, -2.0, 7.0)
    if family == "quarter_turn":
        # s = (x - cx_i) / f up to sign: exactly 0 on the source camera's principal column
        return 0.3, [(_QT, (0.0, 0.0, 0.0)), (_QT.T, (0.0, 0.0, 0.0))], (4.0, 3.0, 0.0)
    if family == "singular":
        # centre exactly on plane 2 (425 + 25 * 2 = 475, exact in fp32): P = I - C n^T / d loses rank
        return 1.2, [(np.eye(3), (0.0, 0.0, D_MIN + D_SCALE * D_INT * 2)),
                     (rot_y(2 * deg), (12.0, 3.0, 0.0))], (3.0, 2.0, 0.0)
    if family == "blind":
        return 1.2, [(rot_y(70 * deg), (8.0, 0.0, 0.0)), (rot_y(-3 * deg), (-14.0, 5.0, 0.0))], (4.0, -3.0, 5.0)
    raise ValueError(family)


def n_own_sources(family):
    return len(_sources(family, 1)[1])


def sample_rig(family, V, h, w):
    """K, R, T (float64 numpy, [V, 3, 3], [V, 3, 3], [V, 3, 1]) of one sample of ``family``: source
    view j is the family's own view j mod n, its centre moved by (j // n) steps so that no two views
    coincide."""
    if family == "zoom":
        from cameras import camera_batch
        assert V == 8 and (h, w) == ZOOM_SHAPE
        K, R, T = (t.double().numpy().copy() for t in camera_batch(1, 8, h, w))
        for j, sc in enumerate(ZOOM_SCALES):
            K[1 + j, :2, :] *= sc
        return K, R, T
    fw, own, step = _sources(family, w)
    K0 = np.array([[fw * w, 0, (w - 1) / 2], [0, fw * w, (h - 1) / 2], [0, 0, 1]], np.float64)
    K, R, T = [K0], [np.eye(3)], [np.zeros((3, 1))]
    for j in range(V - 1):
        Rj, Cj = own[j % len(own)]
        Cj = np.asarray(Cj, np.float64) + (j // len(own)) * np.asarray(step, np.float64)
        Kj = K0.copy()
        if family == "quarter_turn" and w % 2 == 0:
            # an even width has no centre column: the source cameras' principal point moves to column
            # 0, whose normalised coordinate (-1) is exact in fp32 like the centre column's (0)
            Kj[0, 2] = 0.0
        K.append(Kj)
        R.append(Rj)
        T.append(-(Rj @ Cj.reshape(3, 1)))
    return np.stack(K), np.stack(R), np.stack(T)


def rig(families, V, h, w):
    """K, R, T, d_min, d_int (torch fp32, the DataLoader's layouts) of len(families) samples."""
    parts = [sample_rig(f, V, h, w) for f in families]
    K, R, T = (torch.from_numpy(np.concatenate([p[i] for p in parts]).astype(np.float32)) for i in range(3))
    B = len(families)
    d_min = torch.full((B, 1, 1, 1), D_MIN, dtype=torch.float32)
    d_int = torch.full((B, 1, 1, 1), D_INT, dtype=torch.float32)
    return K, R, T, d_min, d_int


def oracle_matrices64(K, R, T, d_min, d_int, B, V, D, h, w):
    """mvs_oracle.sampling_matrices64, or None where torch.inverse refuses a singular homography."""
    import mvs_oracle
    try:
        return mvs_oracle.sampling_matrices64(K, R, T, d_min, d_int, B, V, D, h, w)
    except torch.linalg.LinAlgError:
        return None


def adjugate_matrices(K, R, T, d_min, d_int, B, V, D, h, w, d_begin=0):
    """CPU restatement of csrc/sampling_matrix.h (float64 algebra, both inverses by the adjugate, so a
    singular matrix gives non-finite entries instead of an error), rounded to fp32: [B*V, D, 3, 3].
    Equal to the op's matrices up to fp64 rounding (the device compiler may fuse what numpy does
    not); the GPU tests read the op's own matrices back from its workspace."""
    K, R = K.double().numpy(), R.double().numpy()
    T = T.double().numpy().reshape(-1, 3)
    dm, di = d_min.reshape(-1).numpy().astype(np.float32), d_int.reshape(-1).numpy().astype(np.float32)

    def inv(a):
        a = a.ravel()
        c00, c01, c02 = a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]
        with np.errstate(all="ignore"):
            i = np.float64(1.0) / (a[0] * c00 + a[1] * c01 + a[2] * c02)
            return np.array([c00 * i, (a[2] * a[7] - a[1] * a[8]) * i, (a[1] * a[5] - a[2] * a[4]) * i,
                             c01 * i, (a[0] * a[8] - a[2] * a[6]) * i, (a[2] * a[3] - a[0] * a[5]) * i,
                             c02 * i, (a[1] * a[6] - a[0] * a[7]) * i, (a[0] * a[4] - a[1] * a[3]) * i]).reshape(3, 3)
    sx, sy = 2.0 / (w - 1), 2.0 / (h - 1)
    Nm = np.array([[sx, 0, -1], [0, sy, -1], [0, 0, 1]])
    Ni = np.array([[1 / sx, 0, 1 / sx], [0, 1 / sy, 1 / sy], [0, 0, 1]])
    G = np.empty((B * V, D, 3, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(B * V):
            r = (i // V) * V
            Ci, Cr = -(R[i].T @ T[i]), -(R[r].T @ T[r])
            for k in range(D):
                d = np.float64(f32(dm[i % B] + f32(f32(D_SCALE) * di[i % B]) * f32(d_begin + k)))
                P = np.eye(3) - np.outer(Ci - Cr, R[r][:, 2]) / d
                H = (K[i] @ R[i]) @ (P @ (R[r].T @ inv(K[r])))
                G[i, k] = inv(Nm @ (H @ Ni)).astype(np.float32)
    return G


# ----------------------------------------------------------------------------------------------
# the sampling law on any coordinate
# ----------------------------------------------------------------------------------------------
def coords(G9, h, w):
    """The fp32 law's sampling coordinates (ix, iy) and homogeneous coordinate s of every pixel, [h, w],
    for one 3 x 3 matrix (non-finite entries allowed)."""
    xn, yn = norm_coord(w)[None, :], norm_coord(h)[:, None]
    g = np.asarray(G9, np.float32).ravel()
    with np.errstate(all="ignore"):
        ix, iy = sample_coord(g, xn, yn, h, w)
        s = fma32(yn, g[7], xn * g[6]) + g[8]
    return ix, iy, s


def inside(ix, iy, h, w):
    """Valid samples: at least one of the four taps can lie in the image.  NaN compares false."""
    with np.errstate(invalid="ignore"):
        return (ix >= -1) & (ix < w) & (iy >= -1) & (iy < h)


def sample_law_ext(img, ix, iy):
    """test_sampling_law.sample_law extended to every coordinate as the kernels define it
    (common.h src_coords / make_taps): a sample is exactly 0 unless ix in [-1, w) and iy in [-1, h);
    a NaN or infinite coordinate is outside.  On finite coordinates this is sample_law itself (all
    four taps of such a sample are outside the image, so its sum is 0 there too)."""
    c, h, w = img.shape
    ok = inside(ix, iy, h, w)
    out = sample_law(img, np.where(ok, ix, f32(0)).astype(np.float32), np.where(ok, iy, f32(0)).astype(np.float32))
    return np.where(ok[None], out, f32(0)).astype(np.float32)


def warp_law(feat, G, h, w):
    """The warped volume [N, C, D, h, w] by the extended law, and the valid mask [N, D, h, w]."""
    N, D = G.shape[:2]
    fe = np.asarray(feat, np.float32)
    out = np.empty((N, fe.shape[1], D, h, w), np.float32)
    ok = np.empty((N, D, h, w), bool)
    for i in range(N):
        for k in range(D):
            ix, iy, _ = coords(G[i, k], h, w)
            out[i, :, k] = sample_law_ext(fe[i], ix, iy)
            ok[i, k] = inside(ix, iy, h, w)
    return out, ok


# ----------------------------------------------------------------------------------------------
# per-rig statistics and preconditions (CPU)
# ----------------------------------------------------------------------------------------------
def view_stats(G, h, w):
    """Per (image, plane) of G [N, D, 3, 3]: share of valid samples, share of s < 0, number of
    pixels with |s| <= 1e-8, and s itself [N, D, h, w]."""
    N, D = G.shape[:2]
    ins, neg, tiny = np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, D), np.int64)
    s_all = np.empty((N, D, h, w), np.float32)
    for i in range(N):
        for k in range(D):
            ix, iy, s = coords(G[i, k], h, w)
            ins[i, k] = inside(ix, iy, h, w).mean()
            with np.errstate(invalid="ignore"):
                neg[i, k] = (s < 0).mean()
                tiny[i, k] = int((np.abs(s) <= f32(1e-8)).sum())
            s_all[i, k] = s
    return {"inside": ins, "neg": neg, "tiny": tiny, "s": s_all}


def tiles(h, w):
    for ty in range(0, h, TILE_H):
        for tx in range(0, w, TILE_W):
            yield tx, ty, min(tx + TILE_W, w) - 1, min(ty + TILE_H, h) - 1


def tile_box(G9, px0, py0, px1, py1, h, w):
    """CPU mirror of cost_volume_bwd.hip::tile_box: (x0, y0, x1, y1, pole).  pole: s changes sign over
    the tile's corners or a corner is degenerate, and the box is the whole bordered image."""
    g = np.asarray(G9, np.float32).ravel()
    xs, ys = norm_coord(w), norm_coord(h)
    ix, iy, ss = [], [], []
    with np.errstate(all="ignore"):
        for c in range(4):
            xn, yn = xs[px1 if c & 1 else px0], ys[py1 if c & 2 else py0]
            u = fma32(g[1], yn, fma32(g[0], xn, g[2]))
            v = fma32(g[4], yn, fma32(g[3], xn, g[5]))
            s = fma32(g[7], yn, fma32(g[6], xn, g[8]))
            sc = f32(1) / (s + f32(1e-8))
            ix.append((u * sc + f32(1)) * f32(0.5 * w) - f32(0.5))
            iy.append((v * sc + f32(1)) * f32(0.5 * h) - f32(0.5))
            ss.append(s)
        ix, iy, ss = np.array(ix, np.float32), np.array(iy, np.float32), np.array(ss, np.float32)
        bad = (not (np.abs(ss) > f32(1e-8)).all()) or (not ((np.abs(ix) < 1e7) & (np.abs(iy) < 1e7)).all())
        if bad or ((ss > 0).any() and (ss < 0).any()):
            return -1, -1, w, h, True
        return (max(int(np.floor(ix.min())), -1), max(int(np.floor(iy.min())), -1),
                min(int(np.floor(ix.max())) + 1, w), min(int(np.floor(iy.max())) + 1, h), False)


def box_area(b):
    return 0 if (b[2] < b[0] or b[3] < b[1]) else (b[2] - b[0] + 1) * (b[3] - b[1] + 1)


def pole_tiles(G_view, h, w):
    """Number of (plane, tile) pairs of one source view [D, 3, 3] that take tile_box's pole branch
    because s has both signs on the tile's corners."""
    n = 0
    for k in range(G_view.shape[0]):
        for t in tiles(h, w):
            g = np.asarray(G_view[k], np.float32).ravel()
            xs, ys = norm_coord(w), norm_coord(h)
            with np.errstate(all="ignore"):
                ss = np.array([fma32(g[7], ys[y], fma32(g[6], xs[x], g[8]))
                               for x in (t[0], t[2]) for y in (t[1], t[3])])
                n += bool((ss > 0).any() and (ss < 0).any())
    return n


def tall_tiles(G_view, h, w):
    """Number of (plane, tile) pairs of one source view whose valid tap corners span more rows than
    columns (the staged forward kernel's footprint is then taller than wide)."""
    n = 0
    for k in range(G_view.shape[0]):
        ix, iy, _ = coords(G_view[k], h, w)
        ok = inside(ix, iy, h, w)
        for x0, y0, x1, y1 in tiles(h, w):
            m = ok[y0:y1 + 1, x0:x1 + 1]
            if m.any():
                fx = np.floor(ix[y0:y1 + 1, x0:x1 + 1][m])
                fy = np.floor(iy[y0:y1 + 1, x0:x1 + 1][m])
                n += bool(fy.max() - fy.min() > fx.max() - fx.min())
    return n


def subset_split_tiles(G_sample, h, w):
    """Tiles of one sample [V, D, 3, 3] where the backward's view-subset loop splits: the source
    views' largest single-plane boxes (over the planes of a 32-plane group) sum to more than the LDS
    slots.  Returns (number of such tiles, the largest sum)."""
    V, D = G_sample.shape[:2]
    n, top = 0, 0
    for t in tiles(h, w):
        for k0 in range(0, D, BWD_PLANES):
            tot = sum(max(box_area(tile_box(G_sample[v, k], *t, h, w)) for k in range(k0, min(k0 + BWD_PLANES, D)))
                      for v in range(1, V))
            n += tot > BWD_SLOTS
            top = max(top, tot)
    return n, top


def check_preconditions(family, G_sample, h, w, own_only=True):
    """Assert the family's preconditions on one sample's matrices [V, D, 3, 3] (fp32) and return the
    measured shares.  Only the family's own source views are bound by them (cycled copies at other
    centres are extra views); a precondition that fails is fixed by moving the cameras."""
    V, D = G_sample.shape[:2]
    n_own = min(V - 1, n_own_sources(family)) if family != "zoom" else V - 1
    st = view_stats(G_sample[1:1 + n_own], h, w)
    ins, neg, tiny, s = st["inside"], st["neg"], st["tiny"], st["s"]
    rec = {"inside_min": float(ins.min()), "inside_max": float(ins.max()), "neg_min": float(neg.min()),
           "neg_max": float(neg.max())}
    if family == "roll":
        assert (ins.mean(1) >= 0.5).all(), ins
        for v in range(n_own):
            if v in (0, 2):   # the 90 and 270 degree views
                assert tall_tiles(G_sample[1 + v], h, w) >= 1, v
    elif family == "pole":
        assert (neg.mean(1) >= 0.1).all(), neg
        assert (ins.mean(1) >= 0.3).all(), ins
        rec["pole_tiles"] = [pole_tiles(G_sample[1 + v], h, w) for v in range(n_own)]
        assert sum(rec["pole_tiles"]) >= 1
    elif family == "behind":
        # view 1's centre lies between the planes: s < 0 on the whole image before it, > 0 after it
        assert neg[0, 0] == 1.0 and neg[0, -1] == 0.0, neg
        flip = int(np.argmin(neg[0]))
        assert (neg[0, :flip] == 1.0).all() and (neg[0, flip:] == 0.0).all() and 0 < flip < D
        assert ins[0, :flip].max() > 0 and ins[0, flip:].max() > 0, ins
    elif family == "quarter_turn":
        assert (tiny >= h).all(), tiny   # the principal column of the source camera: s = 0 there
        rec["tiny_min"] = int(tiny.min())
    elif family == "singular":
        assert (ins[0, 2] == 0.0), ins          # every sample of (view 1, plane 2) is invalid
        assert not np.isfinite(G_sample[1, 2]).all()
        assert all(ins[0, k] > 0 for k in range(D) if k != 2), ins
        assert (ins[1:] > 0).all()
    elif family == "blind":
        assert (ins[0] == 0.0).all(), ins       # view 1 sees nothing on any plane
        assert (ins[1:] > 0.5).all(), ins
    elif family == "zoom":
        rec["split_tiles"], rec["largest_box_sum"] = subset_split_tiles(G_sample, h, w)
        assert rec["split_tiles"] >= 1 and rec["largest_box_sum"] > BWD_SLOTS
    else:
        raise ValueError(family)
    return rec


# ----------------------------------------------------------------------------------------------
# the backward's reference: the kernel's own taps, everything else in float64
# ----------------------------------------------------------------------------------------------
def shared_taps(G, h, w):
    """Per (image, plane, pixel): the four tap indices into the flattened source image (y * w + x;
    0 for a tap outside the image) and their fp32 weights (common.h tap_weights order nw, ne, sw,
    se; 0 for a tap outside the image or an invalid sample), from the exact fp32 law on G
    [N, D, 3, 3].  Returns (idx int64 [N, D, 4, h*w], wt float64 [N, D, 4, h*w])."""
    N, D = G.shape[:2]
    idx = np.zeros((N, D, 4, h * w), np.int64)
    wt = np.zeros((N, D, 4, h * w), np.float64)
    for i in range(N):
        for k in range(D):
            ix, iy, _ = coords(G[i, k], h, w)
            ok = inside(ix, iy, h, w)
            ix, iy = np.where(ok, ix, f32(0)).astype(np.float32), np.where(ok, iy, f32(0)).astype(np.float32)
            fx, fy = np.floor(ix), np.floor(iy)
            wx, wy = (ix - fx).astype(np.float32), (iy - fy).astype(np.float32)
            ex, ny = f32(1) - wx, f32(1) - wy
            w4 = [ny * ex, ny * wx, wy * ex, wy * wx]
            for t in range(4):
                xx, yy = fx + (t & 1), fy + (t >> 1)
                good = ok & (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                idx[i, k, t] = np.where(good, yy * w + xx, 0).astype(np.int64).ravel()
                wt[i, k, t] = np.where(good, w4[t], f32(0)).astype(np.float64).ravel()
    return idx, wt


def shared_tap_gradient(feat, G, g, B, V):
    """Reference gradient of <cost volume, g> w.r.t. feat with the kernel's taps held constant:
    sampling, variance and backward in float64 torch.  Also A, the same scatter with every
    contribution |weight * 2/V g (x_v - mean)| in place of the signed one (the yardstick of the
    elementwise bound).  feat [B*V, C, h, w], G [B*V, D, 3, 3], g [B, C, D, h, w];
    returns (grad, A) float64 [B*V, C, h, w]."""
    N, C, h, w = feat.shape
    D = G.shape[1]
    idx, wt = shared_taps(np.asarray(G, np.float32), h, w)
    idx, wt = torch.from_numpy(idx), torch.from_numpy(wt)
    f = feat.detach().double().reshape(N, C, h * w).clone().requires_grad_(True)
    g = g.detach().double().reshape(B, C, D, h * w)

    def sample(i):   # [C, D, hw]
        return sum(f[i][:, idx[i, :, t]] * wt[i, :, t] for t in range(4))
    x = torch.stack([torch.stack([sample(b * V + v) for v in range(V)]) for b in range(B)])   # [B, V, C, D, hw]
    mean = x.mean(1, keepdim=True)
    cv = ((x - mean) ** 2).mean(1)
    cv.backward(g)
    with torch.no_grad():
        coef = (2.0 / V) * g.unsqueeze(1) * (x - mean)        # d <cv, g> / d x_v
        A = torch.zeros(N, C, h * w, dtype=torch.float64)
        for i in range(N):
            c = coef[i // V, i % V].abs()
            for t in range(4):
                A[i].index_add_(1, idx[i, :, t].reshape(-1), (c * wt[i, :, t]).reshape(C, -1))
    return f.grad.reshape(N, C, h, w), A.reshape(N, C, h, w)


def regions(n, pad):
    """The regions the fused head works on for a (D, h, w) volume with padding ``pad``: conv_1_0's
    output region, and the box of the split volume that conv_2_0 reads (lo, hi)."""
    from mvs_amd import model as M
    full = tuple((0, d - 1) for d in n)
    B = M._tconv_input_region(full, n, pad)
    C2 = M._tconv_input_region(B, n, pad)
    h1, h2 = M._grow(B, n, 1), M._grow(C2, n, 1)
    lo = [max(2 * a - p, 0) for (a, _), p in zip(h2, pad)]
    hi = [min(2 * b - p + 2, d - 1) + 1 for (_, b), p, d in zip(h2, pad, n)]
    return h1, lo, hi
