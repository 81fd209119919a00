"""GPU: the fused point cloud (csrc/depth_fuse.hip through mvs_amd.fusion) against the float64 restatement of its
rule (tests/fused_cloud_ref.py, fed the same fp32 inputs widened) on the plane scenes of tests/fusion_cases.py, with
known answers, repeat and stream behaviour, and the public function.

Bounds, derived and not measured:
  emitted, n_merged  equal to the restatement outside the pixels it taints (a slot decision or the absorbed pixel
                     within 1e-9 of flipping, and everything such a pixel could mark; <= 0.1 % of a scene's pixels,
                     none under 1000 pixels: test_fused_cloud_abi.py checks that without a GPU).  The kernel's fp64
                     evaluation differs from numpy's by a few hundred units of 2^-53.
  xyz                within 2^-23 max|coordinate| per point: each coordinate is the float64 value rounded once, at
                     worst the neighbouring fp32 value on a near-tie (the bound of back-projection).
  rgb                within 2^-23 |ref| per channel: likewise one rounding of a float64 mean of values in (0.1, 0.9)."""
import numpy as np
import pytest
import torch

import fused_cloud_ref
import fusion_cases
import fusion_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IDS = lambda c: "%dx%d-N%d-S%d" % c


def _host(a):
    return torch.from_numpy(np.array(a))            # (a copy: the shared scenes are read-only arrays)


def _dev(a):
    return _host(a).to(DEV)


def _fuse_t(sc, depth=None, mask=None, colors=None, pairs=None, K=None, R=None, T=None, **kw):
    """The op's four device tensors for a scene (any input replaced), by the steps fused_point_cloud takes."""
    from mvs_amd import fusion
    depth = sc["depth"] if depth is None else depth
    mask = sc["mask"] if mask is None else mask
    n = depth.shape[0]
    table = fusion.pair_table(sc["pairs"] if pairs is None else pairs, n).to(DEV)
    K, R, T = (_dev(sc[k] if v is None else v) for k, v in (("K", K), ("R", R), ("T", T)))
    mats = fusion.view_pair_matrices(K, R, T.reshape(n, 3), table)
    out = fusion.fuse_views_op(_dev(depth), _dev(mask), None if colors is None else _dev(colors), K, R, T, table,
                               mats, float(kw.get("px_thresh", 1.0)), float(kw.get("rel_thresh", 0.01)))
    em, cnt, xyz, rgb = out
    h, w = depth.shape[2:]
    assert em.shape == cnt.shape == (n, h, w) and em.dtype == torch.bool and cnt.dtype == torch.int32
    assert xyz.shape == (n, h, w, 3) and xyz.dtype == torch.float32
    assert rgb.shape == ((0,) if colors is None else (n, h, w, 3)) and rgb.dtype == torch.float32
    assert not any(t.requires_grad for t in out)
    return out


def _fuse(sc, **kw):
    return tuple(t.cpu().numpy() for t in _fuse_t(sc, **kw))


def _check(got, ref, what):
    """got = the op's (emitted, n_merged, xyz, rgb) arrays, ref = the restatement's five."""
    em, cnt, xyz, rgb = got
    r_em, r_cnt, r_xyz, r_rgb, taint = ref
    assert taint.mean() <= 1e-3 and (taint.size >= 1000 or not taint.any()), (what, taint.mean())
    keep = ~taint
    bad = ((em != r_em) | (cnt != r_cnt)) & keep
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    lim = 2.0 ** -23 * np.abs(r_xyz).max(-1, keepdims=True)
    err = np.abs(xyz.astype(np.float64) - r_xyz)
    print("%s: emitted %d, taint %d, max xyz err / bound %.3g" % (what, int(em.sum()), int(taint.sum()),
                                                                 float((err / np.maximum(lim, 1e-300))[keep].max())))
    assert (err <= lim)[keep].all(), (what, float((err - lim)[keep].max()))
    assert (xyz[~em] == 0).all() and (cnt[~em] == 0).all()
    if r_rgb is not None:
        err = np.abs(rgb.astype(np.float64) - r_rgb)
        lim = 2.0 ** -23 * np.abs(r_rgb)
        print("%s: max rgb err / bound %.3g" % (what, float((err / np.maximum(lim, 1e-300))[keep].max())))
        assert (err <= lim)[keep].all(), (what, float((err - lim)[keep].max()))
        assert (rgb[~em] == 0).all()


def _ref(sc, *names):
    return tuple(sc[k] for k in names)


@pytest.mark.parametrize("case", fusion_cases.SCENES, ids=IDS)
def test_fusion_matches_the_float64_restatement(case):
    sc = fused_cloud_ref.fused_scene(*case)
    with_c = _fuse(sc, colors=sc["colors"])
    _check(with_c, _ref(sc, "emitted", "n_merged", "xyz", "rgb", "taint"), "%s colours" % (case,))
    without = _fuse(sc)
    _check(without, _ref(sc, "emitted", "n_merged", "xyz") + (None, sc["taint"]), str(case))
    # the colours change nothing else; a uint8 mask is the bool mask
    assert all(np.array_equal(a, b) for a, b in zip(with_c[:3], without[:3]))
    as_bytes = _fuse(sc, mask=sc["mask"].astype(np.uint8) * 7)
    assert all(np.array_equal(a, b) for a, b in zip(as_bytes[:3], without[:3]))
    if case in ((128, 160, 5, 4), (17, 40, 5, 10)):
        assert without[0].sum() < 0.35 * sc["mask"].sum()          # it de-duplicates


@pytest.mark.parametrize("hw", ((1, 1), (5, 7), (17, 40), (128, 160)))
def test_no_sources_emits_the_mask(hw):
    """N = 1, and N = 5 with every slot empty: emitted == mask & (depth > 0), nothing merged, and the points are
    point_cloud's within the back-projection bound (two roundings of the same float64 point)."""
    from mvs_amd import fusion
    h, w = hw
    rng = np.random.default_rng(h * w)
    for n, pairs in ((1, [[0]]), (5, [[-1, 0], [1], [], [3, -1, 3], [4]])):
        K, R, T = fusion_ref.arc_cameras(n, h, w)
        depth = fusion_ref.plane_depths(K, R, T, h, w)
        mask = rng.uniform(size=depth.shape) < 0.7
        if h * w > 4:
            depth[n - 1, 0, h // 2, w // 2], mask[n - 1, 0, h // 2, w // 2] = -4.0, True
        sc = {"K": K, "R": R, "T": T, "depth": depth, "mask": mask, "pairs": pairs}
        em, cnt, xyz, _ = _fuse(sc)
        want = mask[:, 0] & (depth[:, 0] > 0)
        assert np.array_equal(em, want) and (cnt == 0).all()
        cams = [_host(a) for a in (K, R, T)]
        pts = fusion.fused_point_cloud(_dev(depth), _dev(mask), *cams, pairs).cpu().numpy()
        ref = fusion.point_cloud(_dev(depth), _dev(mask & (depth > 0)), *cams).cpu().numpy()
        assert pts.shape == ref.shape == (int(want.sum()), 3) and np.array_equal(pts, xyz[em])
        lim = 2.0 ** -23 * np.abs(ref.astype(np.float64)).max(-1, keepdims=True)
        assert (np.abs(pts.astype(np.float64) - ref) <= lim).all()


def test_empty_first_view_marks_nothing():
    """mask[0] all false: view 0 emits nothing and marks nothing, so the later views emit what a run over views
    1 .. N-1 alone emits (view 0 still serves as a source: the merge counts may differ, the flags may not)."""
    sc = fused_cloud_ref.fused_scene(17, 40, 5, 10)
    mask = sc["mask"].copy()
    mask[0] = False
    em, cnt, xyz, _ = _fuse(sc, mask=mask)
    assert not em[0].any() and (cnt[0] == 0).all() and (xyz[0] == 0).all()
    rest = [[v - 1 if v >= 1 else -1 for v in row] for row in sc["pairs"][1:]]
    sub = {"K": sc["K"][1:], "R": sc["R"][1:], "T": sc["T"][1:], "depth": sc["depth"][1:], "mask": mask[1:],
           "pairs": rest}
    em_sub = _fuse(sub)[0]
    assert np.array_equal(em[1], mask[1, 0]) and np.array_equal(em[1], em_sub[0])
    assert np.array_equal(em[1:], em_sub)
    assert em[1].sum() > sc["emitted"][1].sum()                       # with view 0 present, view 1 emitted far less
    ref = fused_cloud_ref.fuse(sc["depth"], mask, None, sc["K"], sc["R"], sc["T"], sc["table"])
    _check((em, cnt, xyz, None), ref, "empty first view")


def test_hole_in_a_source_map():
    """A rectangle of zeros in view 1's map: the pixels of view 0 whose four taps touch it merge nothing (their one
    slot is view 1), and view 1's pixels that only those would have absorbed are emitted."""
    sc = fused_cloud_ref.fused_scene(128, 160, 2, 1)
    depth = sc["depth"].copy()
    depth[1, 0, 40:70, 50:100] = 0.0
    mask = depth > 0
    got = _fuse(sc, depth=depth, mask=mask, colors=sc["colors"])
    ref = fused_cloud_ref.fuse(depth, mask, sc["colors"], sc["K"], sc["R"], sc["T"], sc["table"])
    _check(got, ref, "hole")
    em, cnt = got[:2]
    M, m = fusion_ref.pair_matrix(sc["K"], sc["R"], sc["T"], 0, 1)
    ys, xs = np.meshgrid(np.arange(128.0), np.arange(160.0), indexing="ij")
    d = depth[0, 0].astype(np.float64)
    p = d * np.einsum("ij,jhw->ihw", M, np.stack([xs, ys, np.ones_like(xs)])) + m.reshape(3, 1, 1)
    x0, y0 = np.floor(p[0] / p[2]), np.floor(p[1] / p[2])
    touches = (x0 + 1 >= 50) & (x0 <= 99) & (y0 + 1 >= 40) & (y0 <= 69)
    assert touches.sum() > 1000 and em[0].all() and (cnt[0][touches] == 0).all()
    whole = _fuse(sc, mask=sc["depth"] > 0)
    assert np.array_equal(cnt[0][~touches], whole[1][0][~touches]) and (cnt[0][~touches] == 1).sum() > 10000
    assert not em[1, 40:70, 50:100].any()                              # invalid pixels are never emitted
    assert em[1].sum() > whole[0][1].sum()                              # fewer of view 1's pixels were absorbed


def test_scaled_source_merges_nowhere():
    """View 1's map scaled by 1.05 against the 1 % gate, each of views 0 and 1 the other's only source: nothing
    merges, nothing is absorbed, emitted == mask everywhere."""
    sc = fused_cloud_ref.fused_scene(17, 40, 5, 10)
    depth = sc["depth"].copy()
    depth[1] *= np.float32(1.05)
    mask = np.random.default_rng(3).uniform(size=depth.shape) < 0.8
    only = [[1], [0], [], [], []]
    em, cnt, xyz, rgb = _fuse(sc, depth=depth, mask=mask, colors=sc["colors"], pairs=only)
    assert np.array_equal(em, mask[:, 0]) and (cnt == 0).all()
    want = np.where(mask, sc["colors"], np.float32(0.0)).transpose(0, 2, 3, 1)
    assert np.array_equal(rgb, want)                                    # a pixel's own colour, bit for bit
    em, cnt, _, _ = _fuse(sc, mask=mask, pairs=only)                    # unscaled, the same slot merges
    assert cnt[0].sum() > 0 and em[1].sum() < mask[1].sum()


@pytest.mark.parametrize("case", [(9, 33, 5, 4), (17, 40, 5, 10), (128, 160, 5, 4)], ids=IDS)
def test_reversed_view_order(case):
    """The scene with its views in the opposite order (cameras, maps, mask, colours and pairs permuted) gives the
    restatement's result for that scene -- and not the forward result permuted: the first view emits its mask."""
    sc = fused_cloud_ref.fused_scene(*case)
    n = case[2]
    rev = {k: np.ascontiguousarray(sc[k][::-1]) for k in ("K", "R", "T", "depth", "mask", "colors")}
    rev["pairs"] = fused_cloud_ref.reversed_pairs(sc["pairs"], n)
    got = _fuse(rev, colors=rev["colors"])
    ref = fused_cloud_ref.fuse(rev["depth"], rev["mask"], rev["colors"], rev["K"], rev["R"], rev["T"],
                               fusion_ref.pad_pairs(rev["pairs"]))
    _check(got, ref, "%s reversed" % (case,))
    assert np.array_equal(got[0][0], rev["mask"][0, 0])
    assert not np.array_equal(got[0][::-1], sc["emitted"])


def test_repeat_stream_and_dirty_workspace():
    from mvs_amd import _lib, fusion
    sc = fused_cloud_ref.fused_scene(128, 160, 5, 4)
    first = _fuse_t(sc, colors=sc["colors"])
    again = _fuse_t(sc, colors=sc["colors"])
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = _fuse_t(sc, colors=sc["colors"])
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, on_side))
    # the C entry with a workspace full of ones: the call zeroes it before the first view
    lib = _lib.load()
    n, _, h, w = sc["depth"].shape
    table = fusion.pair_table(sc["pairs"], n).to(DEV)
    K, R, T = _dev(sc["K"]), _dev(sc["R"]), _dev(sc["T"]).reshape(n, 3).contiguous()
    mats = fusion.view_pair_matrices(K, R, T, table)
    depth, mask, colors = _dev(sc["depth"]), _dev(sc["mask"]), _dev(sc["colors"])
    assert lib.mvs_fuse_views_workspace_bytes(n, h, w) == n * h * w
    used = torch.ones(n * h * w, dtype=torch.uint8, device=DEV)
    em = torch.empty((n, h, w), dtype=torch.bool, device=DEV)
    cnt = torch.empty((n, h, w), dtype=torch.int32, device=DEV)
    xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=DEV)
    rgb = torch.empty((n, h, w, 3), dtype=torch.float32, device=DEV)
    st = lib.mvs_fuse_views_fwd(*(_lib.ptr(t) for t in (depth, mask, colors, K, R, T, table, mats)), n, table.shape[1],
                                h, w, 1.0, 0.01, *(_lib.ptr(t) for t in (used, em, cnt, xyz, rgb)),
                                _lib.stream_handle(DEV))
    assert st == 0
    assert all(torch.equal(a, b) for a, b in zip(first, (em, cnt, xyz, rgb)))
    # afterwards the workspace holds the marks: every kept pixel that was not emitted carries one
    marks = used.reshape(n, h, w).bool()
    kept = mask[:, 0] & (depth[:, 0] > 0)
    assert not (kept & ~em & ~marks).any() and marks[1:].any() and not marks.all()


def test_public_function():
    from mvs_amd import fusion
    sc = fused_cloud_ref.fused_scene(17, 40, 5, 10)
    em, cnt, xyz, rgb = _fuse_t(sc, colors=sc["colors"])
    m = int(em.sum())
    depth, mask = _dev(sc["depth"]).requires_grad_(True), _dev(sc["mask"])
    cams = [_host(sc[k]) for k in "KRT"]
    colors = _dev(sc["colors"]).requires_grad_(True)
    pts = fusion.fused_point_cloud(depth, mask, *cams, sc["pairs"])
    assert isinstance(pts, torch.Tensor) and pts.shape == (m, 3) and pts.dtype == torch.float32
    idx = em.nonzero()                                                   # view, row, column order
    assert torch.equal(pts, xyz[em]) and torch.equal(pts, xyz[idx[:, 0], idx[:, 1], idx[:, 2]])
    pts2, col = fusion.fused_point_cloud(depth, mask, *cams, sc["pairs"], colors=colors)
    assert torch.equal(pts2, pts) and col.shape == (m, 3) and col.dtype == torch.float32
    assert torch.equal(col, rgb[em])
    pts3, n3 = fusion.fused_point_cloud(depth, mask, *cams, _host(sc["table"]), return_counts=True)
    assert torch.equal(pts3, pts) and n3.shape == (m,) and n3.dtype == torch.int32 and torch.equal(n3, cnt[em])
    pts4, col4, n4 = fusion.fused_point_cloud(depth, mask, *cams, sc["pairs"], colors=colors, return_counts=True)
    assert torch.equal(pts4, pts) and torch.equal(col4, col) and torch.equal(n4, n3)
    assert not any(t.requires_grad for t in (pts, col, n3))
    assert m < 0.35 * fusion.point_cloud(depth, mask, *cams).shape[0]    # fewer points than point_cloud's
    with pytest.raises(ValueError):
        fusion.fused_point_cloud(depth, mask.to(torch.uint8), *cams, sc["pairs"])
    with pytest.raises(ValueError):
        fusion.fused_point_cloud(depth, mask, *cams, sc["pairs"], colors=colors[:, :2])
    with pytest.raises(ValueError):
        fusion.fused_point_cloud(depth, mask, *cams, sc["pairs"], px_thresh=0.0)
