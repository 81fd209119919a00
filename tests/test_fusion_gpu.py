"""GPU: the depth-map filtering kernels (csrc/depth_filter.hip through mvs_amd.fusion) against the float64
restatement of their definitions (tests/fusion_ref.py, fed the same fp32 inputs widened), on plane scenes
(tests/fusion_cases.py), with known answers, and MVSNet.forward_with_confidence against forward.

Bounds, derived and not measured:
  n_consistent  equal to the restatement outside the pixels it marks near a decision (<= 0.1 % of a scene's pixels,
                none under 1000 pixels: test_fusion_abi.py checks that without a GPU).
  depth_avg     within 2^-23 |ref|: the kernel's fp64 evaluation differs from the restatement's by a few hundred units
                of 2^-53, so the output is the float64 value rounded once to fp32, at worst the neighbouring fp32
                value on a near-tie.
  confidence    within 4 * 2^-24 conf: three fp32 adds of non-negative terms; pixels whose float64 t is within 1e-4 of
                an integer are left out (<= 1 % by construction of the depths).
  back-project  within 2^-23 max|coordinate| per point of float64 (one rounding of each coordinate)."""
import numpy as np
import pytest
import torch

import fusion_cases
import fusion_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = ((1, 1), (2, 2), (5, 7), (9, 33), (17, 40), (128, 160))


def _host(a):
    return torch.from_numpy(np.array(a))            # (a copy: the shared scenes are read-only arrays)


def _dev(a):
    return _host(a).to(DEV)


def _run(sc, depth=None, K=None, R=None, T=None, pairs=None, **kw):
    from mvs_amd import fusion
    depth = sc["depth"] if depth is None else depth
    cnt, avg = fusion.geometric_consistency(_dev(depth), _host(sc["K"] if K is None else K),
                                            _host(sc["R"] if R is None else R), _host(sc["T"] if T is None else T),
                                            sc["pairs"] if pairs is None else pairs, **kw)
    assert cnt.dtype == torch.int32 and avg.dtype == torch.float32 and cnt.shape == avg.shape == depth.shape
    assert not cnt.requires_grad and not avg.requires_grad
    return cnt.cpu().numpy(), avg.cpu().numpy()


def _check(got_cnt, got_avg, ref_cnt, ref_avg, near, what):
    keep = ~near
    assert near.mean() <= 1e-3 and (near.size >= 1000 or not near.any()), (what, near.mean())
    bad = (got_cnt != ref_cnt) & keep
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    err = np.abs(got_avg.astype(np.float64) - ref_avg)
    lim = 2.0 ** -23 * np.abs(ref_avg)
    print("%s: near %d of %d, max depth_avg err / |ref| %.3g" % (what, int(near.sum()), near.size,
                                                                   float((err / np.maximum(np.abs(ref_avg), 1e-300))[keep].max())))
    assert (err <= lim)[keep].all(), (what, float((err - lim)[keep].max()))


@pytest.mark.parametrize("case", fusion_cases.SCENES, ids=lambda c: "%dx%d-N%d-S%d" % c)
def test_consistency_matches_the_float64_restatement(case):
    sc = fusion_cases.scene(*case)
    cnt, avg = _run(sc)
    _check(cnt, avg, sc["count"], sc["avg"], sc["near"], str(case))
    slots = fusion_ref.non_empty_slots(sc["table"])
    assert (cnt <= slots.reshape(-1, 1, 1, 1)).all()
    if case in fusion_cases.FULL_COUNT:
        # the scene shows something: the restatement itself counts every non-empty slot on most interior pixels
        share = fusion_cases.full_count_share(sc)
        print("%s: full count on %.4f of the interior pixels" % (case, share))
        assert share > fusion_cases.FULL_COUNT_SHARE, share
    # a CPU integer tensor with -1 padding is the same call as the ragged list
    cnt2, avg2 = _run(sc, pairs=_host(sc["table"]))
    assert np.array_equal(cnt, cnt2) and np.array_equal(avg.view(np.int32), avg2.view(np.int32))


def test_scaled_source_is_consistent_nowhere():
    """View 1's map scaled by 1.05: a 5 % depth error against the 1 % gate.  Seen from view 0, slot 0 (view 1) never
    counts -- whichever point of the scaled map the pixel meets; as a reference view, view 1 agrees with nobody."""
    sc = fusion_cases.scene(17, 40, 5, 10)
    depth = sc["depth"].copy()
    depth[1] *= np.float32(1.05)
    ref_cnt, ref_avg, near = fusion_ref.consistency(depth, sc["K"], sc["R"], sc["T"], sc["table"])
    cnt, avg = _run(sc, depth=depth)
    _check(cnt, avg, ref_cnt, ref_avg, near, "scaled")
    assert (cnt[1] == 0).all() and np.array_equal(avg[1], depth[1])
    only = [[1], [0], [], [], []]
    cnt, avg = _run(sc, depth=depth, pairs=only)
    assert (cnt == 0).all() and np.array_equal(avg.view(np.int32), depth.view(np.int32))
    cnt, _ = _run(sc, pairs=only)                                  # unscaled, the same slot is consistent
    assert cnt[0].sum() > 0 and cnt[1].sum() > 0


def test_hole_in_a_source_map():
    """A rectangle of zeros in view 1's map: no pixel of view 0 whose four taps touch it counts that slot, the
    others keep their count; view 1's own pixels inside it get 0 in both outputs."""
    sc = fusion_cases.scene(128, 160, 2, 1)
    depth = sc["depth"].copy()
    depth[1, 0, 40:70, 50:100] = 0.0
    ref_cnt, ref_avg, near = fusion_ref.consistency(depth, sc["K"], sc["R"], sc["T"], sc["table"])
    cnt, avg = _run(sc, depth=depth)
    _check(cnt, avg, ref_cnt, ref_avg, near, "hole")
    # where view 0's pixels land in view 1, by the restatement's own step 1
    M, m = fusion_ref.pair_matrix(sc["K"], sc["R"], sc["T"], 0, 1)
    ys, xs = np.meshgrid(np.arange(128.0), np.arange(160.0), indexing="ij")
    d = depth[0, 0].astype(np.float64)
    p = d * np.einsum("ij,jhw->ihw", M, np.stack([xs, ys, np.ones_like(xs)])) + m.reshape(3, 1, 1)
    x0, y0 = np.floor(p[0] / p[2]), np.floor(p[1] / p[2])
    touches = (x0 + 1 >= 50) & (x0 <= 99) & (y0 + 1 >= 40) & (y0 <= 69)
    assert touches.sum() > 1000 and (cnt[0, 0][touches] == 0).all()
    whole = fusion_cases.scene(128, 160, 2, 1)["count"]
    assert np.array_equal(cnt[0, 0][~touches], whole[0, 0][~touches])
    assert (cnt[1, 0, 40:70, 50:100] == 0).all() and (avg[1, 0, 40:70, 50:100] == 0).all()


def test_source_facing_away_is_never_consistent():
    """View 1 turned by half a turn about its own y axis (same centre): every point of view 0 is behind it, p.z <= 0."""
    sc = fusion_cases.scene(17, 40, 2, 1)
    flip = np.diag([-1.0, 1.0, -1.0]).astype(np.float32)
    R, T = sc["R"].copy(), sc["T"].copy()
    R[1], T[1] = flip @ R[1], flip @ T[1]
    ref_cnt, _, _ = fusion_ref.consistency(sc["depth"], sc["K"], R, T, sc["table"])
    assert (ref_cnt[0] == 0).all() and sc["count"][0].sum() > 0
    cnt, avg = _run(sc, R=R, T=T)
    assert (cnt[0] == 0).all() and np.array_equal(avg[0], sc["depth"][0])


@pytest.mark.parametrize("hw", SHAPES)
def test_no_sources_returns_the_input(hw):
    """N = 1, and N = 5 with every slot empty (-1, or the view itself): 0 counts and the input depth, bit for bit, on
    the valid pixels; 0 on the others."""
    h, w = hw
    sc = fusion_cases.scene(h, w, 1, 1)
    cnt, avg = _run(sc)
    assert (cnt == 0).all() and np.array_equal(avg.view(np.int32), sc["depth"].view(np.int32))
    K, R, T = fusion_ref.arc_cameras(5, h, w)
    depth = fusion_ref.plane_depths(K, R, T, h, w)
    depth[3, 0, h // 2, w // 2] = -4.0
    sc5 = {"K": K, "R": R, "T": T, "depth": depth}
    cnt, avg = _run(sc5, pairs=[[-1, 0], [1], [], [3, -1, 3], [4]])
    want = np.where(depth > 0, depth, np.float32(0.0))
    assert (cnt == 0).all() and np.array_equal(avg.view(np.int32), want.view(np.int32))


def test_invalid_pixels_of_the_view_itself():
    """A NaN, a 0 and a negative depth in view 0's own map: 0 in both outputs there, the neighbours untouched (views
    that use view 0 as a source change only where their taps meet those pixels: the restatement says where)."""
    sc = fusion_cases.scene(17, 40, 5, 10)
    depth = sc["depth"].copy()
    spots = ((3, 5), (8, 20), (12, 33))
    for (y, x), v in zip(spots, (np.nan, 0.0, -500.0)):
        depth[0, 0, y, x] = v
    ref_cnt, ref_avg, near = fusion_ref.consistency(depth, sc["K"], sc["R"], sc["T"], sc["table"])
    cnt, avg = _run(sc, depth=depth)
    _check(cnt, avg, ref_cnt, ref_avg, near, "invalid")
    base_cnt, base_avg = _run(sc)
    other = np.ones((17, 40), bool)
    for y, x in spots:
        assert cnt[0, 0, y, x] == 0 and avg[0, 0, y, x] == 0.0
        other[y, x] = False
    assert np.array_equal(cnt[0, 0][other], base_cnt[0, 0][other])
    assert np.array_equal(avg[0, 0][other], base_avg[0, 0][other])


def test_tighter_thresholds_never_raise_a_count():
    sc = fusion_cases.scene(17, 40, 5, 10)
    rng = np.random.default_rng(2)
    depth = (sc["depth"] * (1.0 + 0.004 * rng.standard_normal(sc["depth"].shape))).astype(np.float32)
    last = None
    for px, rel in ((2.0, 0.02), (1.0, 0.02), (1.0, 0.01), (0.5, 0.01), (0.5, 0.004), (0.05, 0.004), (0.05, 1e-4)):
        cnt, _ = _run(sc, depth=depth, px_thresh=px, rel_thresh=rel)
        if last is not None:
            assert (cnt <= last).all(), (px, rel)
        last = cnt
    assert last.sum() < _run(sc, depth=depth, px_thresh=2.0, rel_thresh=0.02)[0].sum()


# ---- photometric confidence ----
def _conf_inputs(B, D, h, w, seed, rows):
    """A softmax-like volume, planes d_0 + step k (per sample when rows == B) and depths spread from below plane 0
    to above plane D - 1 with t away from the integers."""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, 1, D, h, w)) * 3.0
    prob = np.exp(logits - logits.max(2, keepdims=True))
    prob = (prob / prob.sum(2, keepdims=True)).astype(np.float32)
    d0 = 425.0 + 30.0 * np.arange(rows)
    step = 2.5 * (1.0 + 0.37 * np.arange(rows))
    db = (d0[:, None] + step[:, None] * np.arange(D)[None, :]).astype(np.float32)
    k = rng.integers(-2, D + 2, (B, 1, h, w))
    t = k + rng.uniform(0.02, 0.98, (B, 1, h, w))
    full = np.repeat(db, B // rows, 0).astype(np.float64)
    depth = (full[:, 0].reshape(B, 1, 1, 1) + t * (full[:, 1] - full[:, 0]).reshape(B, 1, 1, 1)).astype(np.float32)
    return prob, depth, db


@pytest.mark.parametrize("D", [2, 5, 48])
@pytest.mark.parametrize("B", [1, 3])
def test_confidence_matches_the_float64_restatement(B, D):
    from mvs_amd import fusion
    for i, (h, w) in enumerate(SHAPES):
        prob, depth, db = _conf_inputs(B, D, h, w, seed=100 * D + 10 * B + i, rows=B if i % 2 else 1)
        got = fusion.photometric_confidence(_dev(prob), _dev(depth), _dev(db))
        assert got.shape == (B, 1, h, w) and got.dtype == torch.float32 and not got.requires_grad
        ref, t = fusion_ref.confidence(prob, depth, db)
        keep = np.abs(t - np.rint(t)) >= 1e-4
        assert (~keep).mean() <= 0.01
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        assert (err <= 4.0 * 2.0 ** -24 * ref)[keep].all(), (B, D, h, w, float((err / np.maximum(ref, 1e-30))[keep].max()))
        if db.shape[0] == 1 and B > 1:                              # [1][D] and [B][D] planes agree
            again = fusion.photometric_confidence(_dev(prob), _dev(depth), _dev(np.repeat(db, B, 0)))
            assert torch.equal(got, again)


def test_confidence_known_answers():
    from mvs_amd import fusion
    B, D, h, w, j = 2, 48, 9, 33, 20
    db = (425.0 + 2.5 * np.arange(D, dtype=np.float32)).reshape(1, D)        # exact in fp32: t is the plane index
    prob = np.zeros((B, 1, D, h, w), np.float32)
    prob[:, :, j] = 1.0
    at = lambda k: np.full((B, 1, h, w), db[0, 0] + 2.5 * k, np.float32)
    conf = lambda p, d: fusion.photometric_confidence(_dev(p), _dev(d), _dev(db)).cpu().numpy()
    assert (conf(prob, at(j)) == 1.0).all()
    assert (conf(prob, at(j + 1)) == 1.0).all() and (conf(prob, at(j - 2)) == 1.0).all()   # the window k0-1 .. k0+2
    assert (conf(prob, at(j + 3)) == 0.0).all() and (conf(prob, at(j - 3)) == 0.0).all()   # three planes away
    assert (conf(prob, at(j + 2)) == 0.0).all()
    # clamps: below plane 0 the window is planes 0..2, above plane D-1 it is planes D-2, D-1; added in ascending k
    rng = np.random.default_rng(8)
    p = rng.uniform(0.0, 0.05, (B, 1, D, h, w)).astype(np.float32)
    low = (p[:, :, 0] + p[:, :, 1]) + p[:, :, 2]
    high = p[:, :, D - 2] + p[:, :, D - 1]
    for d in (at(-7.5), at(-0.25), np.full((B, 1, h, w), -np.inf, np.float32)):
        assert np.array_equal(conf(p, d), low)
    for d in (at(D - 1), at(D + 11.5), np.full((B, 1, h, w), np.inf, np.float32)):
        assert np.array_equal(conf(p, d), high)
    inner = ((p[:, :, 4] + p[:, :, 5]) + p[:, :, 6]) + p[:, :, 7]
    assert np.array_equal(conf(p, at(5.5)), inner)
    # a NaN depth: 0 there, the neighbours untouched
    d = at(5.5)
    d[1, 0, 4, 17] = np.nan
    got = conf(p, d)
    assert got[1, 0, 4, 17] == 0.0
    got[1, 0, 4, 17] = inner[1, 0, 4, 17]
    assert np.array_equal(got, inner)


# ---- back-projection, filter_depth, point_cloud ----
@pytest.mark.parametrize("case", [(1, 1, 1, 1), (5, 7, 5, 10), (9, 33, 5, 4), (128, 160, 5, 4)],
                         ids=lambda c: "%dx%d-N%d" % c[:3])
def test_backprojection(case):
    from mvs_amd import fusion
    sc = fusion_cases.scene(*case)
    depth = sc["depth"].copy()
    if depth[0, 0].size > 4:
        depth[0, 0, 1, 2], depth[-1, 0, -1, -1] = 0.0, np.nan
    xyz = fusion.backproject(_dev(depth), *(_host(sc[k]) for k in "KRT"))
    N, _, h, w = depth.shape
    assert xyz.shape == (N, h, w, 3) and xyz.dtype == torch.float32 and not xyz.requires_grad
    got = xyz.cpu().numpy().astype(np.float64)
    ref = fusion_ref.backproject(depth, sc["K"], sc["R"], sc["T"])
    lim = 2.0 ** -23 * np.abs(ref).max(-1, keepdims=True)
    assert (np.abs(got - ref) <= lim).all()
    valid = depth[:, 0] > 0
    assert (got[~valid] == 0.0).all()
    # on the plane, and back through K (R X + T) to (x, y, d).  The fp32 points are within e = sqrt(3) 2^-24 max|X| of
    # the float64 ones; a point moved by e moves its depth by <= e and its pixel by <= 2 f e / d (f / d per unit across
    # the ray, the pixel's own tangent <= 1 along it)
    K, R, T = (sc[k].astype(np.float64) for k in "KRT")
    e = np.sqrt(3.0) * 2.0 ** -24 * np.abs(got).max()
    assert (np.abs(got[valid] @ fusion_ref.PLANE_N - fusion_ref.PLANE_C) <= 2e-4).all()   # fp32 depths: 935 * 2^-24 * 3
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    for n in range(N):
        cam = got[n] @ R[n].T + T[n].reshape(3)
        pix = cam @ K[n].T
        v = valid[n]
        d = depth[n, 0].astype(np.float64)
        assert (np.abs(pix[..., 2] - d)[v] <= e).all()
        tol = 2.0 * K[n, 0, 0] * e / d[v].min()
        assert (np.abs(pix[..., 0] / pix[..., 2] - xs)[v] <= tol).all()
        assert (np.abs(pix[..., 1] / pix[..., 2] - ys)[v] <= tol).all()


def test_filter_depth_and_point_cloud():
    from mvs_amd import fusion
    sc = fusion_cases.scene(17, 40, 5, 10)
    rng = np.random.default_rng(6)
    depth = sc["depth"].copy()
    depth[2, 0, 5:9, 10:20] = 0.0
    N, _, h, w = depth.shape
    conf = _dev(rng.uniform(0.5, 1.0, depth.shape).astype(np.float32))
    colors = _dev(rng.integers(0, 256, (N, 3, h, w)).astype(np.uint8))
    d = _dev(depth)
    cams = [_host(sc[k]) for k in "KRT"]
    cnt, avg = fusion.geometric_consistency(d, *cams, sc["pairs"])
    for kw in ({}, {"conf_thresh": 0.7, "min_consistent": 3}, {"min_consistent": 1, "px_thresh": 0.5}):
        geo = {k: v for k, v in kw.items() if k in ("px_thresh", "rel_thresh")}
        c, a = fusion.geometric_consistency(d, *cams, sc["pairs"], **geo)
        mask, got_avg = fusion.filter_depth(d, conf, *cams, sc["pairs"], **kw)
        want = (d > 0) & (conf >= kw.get("conf_thresh", 0.8)) & (c >= kw.get("min_consistent", 2))
        assert mask.dtype == torch.bool and mask.shape == d.shape and torch.equal(mask, want)
        assert torch.equal(got_avg, a)
    mask_nc, _ = fusion.filter_depth(d, None, *cams, sc["pairs"])
    assert torch.equal(mask_nc, (d > 0) & (cnt >= 2)) and mask_nc.sum() > mask.sum() > 0
    assert not mask_nc[2, 0, 5:9, 10:20].any()
    # the cloud: M == mask.sum(), view / row / column order, colours in step with the points
    pts, col = fusion.point_cloud(avg, mask_nc, *cams, colors=colors)
    M = int(mask_nc.sum())
    assert pts.shape == (M, 3) and col.shape == (M, 3) and pts.dtype == torch.float32 and col.dtype == torch.uint8
    xyz = fusion.backproject(avg, *cams)
    idx = mask_nc[:, 0].nonzero()
    assert torch.equal(pts, xyz[idx[:, 0], idx[:, 1], idx[:, 2]])
    assert torch.equal(col, colors[idx[:, 0], :, idx[:, 1], idx[:, 2]])
    assert torch.equal(fusion.point_cloud(avg, mask_nc, *cams), pts)
    assert fusion.point_cloud(avg, torch.zeros_like(mask_nc), *cams).shape == (0, 3)


# ---- MVSNet.forward_with_confidence ----
def test_forward_with_confidence():
    """Eval mode, fp32, a 36 x 44 feature map (144 x 176 images, 3 views, 32 planes): the two depth maps are
    forward's, bit for bit; the confidence is photometric_confidence of the probability volume the regulariser
    module returned in that forward (a forward hook on the public module) on forward's initial depth map and the
    planes warp_and_assemble_cost_volume returns; its values lie in [0, 1 + 4 * 2^-24]."""
    from cameras import camera_batch, depth_range
    from mvs_amd import fusion, warp_and_assemble_cost_volume
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    B, V, D, H, W = 1, 3, 32, 144, 176
    torch.manual_seed(0)
    net = MVSNet(MVSConfig(d_num=D, in_h=H, in_w=W, arithmetic="fp32")).to(DEV).eval()
    K, R, T = camera_batch(B, V, H // 4, W // 4)
    d_min, d_int = depth_range(B, d_int=0.4)
    img = torch.rand(B * V, 3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    seen = []
    hook = net.cost_volume_reg.register_forward_hook(lambda mod, args, out: seen.append(out))
    try:
        with torch.no_grad():
            ini, ref = net(img, K, R, T, d_min, d_int, B, V)
            ini2, ref2, conf = net.forward_with_confidence(img, K, R, T, d_min, d_int, B, V)
            feats = net.feature_encoder(img)
            _, d_batch, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feats, B, V, d_num=D,
                                                          d_scale=net.cfg.d_scale)
    finally:
        hook.remove()
    assert len(seen) == 2 and tuple(seen[0].shape) == (B, 1, D, H // 4, W // 4) and torch.equal(seen[0], seen[1])
    assert torch.equal(ini, ini2) and torch.equal(ref, ref2)
    assert conf.shape == ini.shape == (B, 1, H // 4, W // 4) and conf.dtype == torch.float32
    assert not conf.requires_grad
    assert torch.equal(conf, fusion.photometric_confidence(seen[0], ini, d_batch))
    assert float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0 + 4.0 * 2.0 ** -24
    assert float(conf.max()) > 0.0
