"""GPU: nearest-neighbour distances between two clouds and the cloud evaluation built on them (csrc/cloud_nn.hip
through mvs_amd.cloud_eval) against the float64 brute-force restatement of the definition
(tests/cloud_eval_ref.py, fed the same fp32 inputs widened), with known answers on integer coordinates, grid
independence, the structures a grid search can go wrong on, repeat and stream behaviour, and evaluate_cloud.

Bounds, derived and not measured:
  dist    +inf exactly where the restatement finds no candidate, outside the queries it flags as near the gate (best,
          or a rejected candidate, within 1e-9 relative of max_dist^2; test_cloud_eval_abi.py checks without a GPU
          that the clouds used here flag none).  Elsewhere within 2^-23 ref: dist is the float64 sqrt(best) rounded
          once to fp32 (half a unit, 2^-24 ref), at worst the neighbouring fp32 value on a near-tie.  Kernel and
          numpy differ before that rounding by a few units of 2^-53: the kernel fuses the products of d2 into two
          FMAs where numpy rounds each product and sum (at most 3 roundings, 2^-53 relative each), and sqrt halves a
          relative error.  With integer coordinates every d2 is exact and the comparison is for equality.
  index   -1 exactly where dist is +inf; elsewhere the restatement's own d2(i, index[i]) is <= its minimum times
          (1 + 1e-12): the kernel may pick another point only where two d2 agree to those few units of 2^-53.
  evaluate_cloud   means within 1e-6 relative: a float64 mean of fp32 values each within 2^-23 of the restatement's
          (1.2e-7), the float64 summation error far below; counts and medians are exact (the restatement rounds its
          distances to fp32 as the kernel does; a last-place difference there would show, and is a finding)."""
import math

import numpy as np
import pytest
import torch

import cloud_eval_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_DIST = ref.MAX_DIST
INF = float("inf")


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).reshape(-1, 3).to(DEV)


def _nearest(query, target, max_dist=MAX_DIST, cell=None):
    from mvs_amd import cloud_eval
    dist, index = cloud_eval.nearest_distance(_dev(query), _dev(target), max_dist, cell)
    m = len(np.asarray(query).reshape(-1, 3))
    assert dist.shape == index.shape == (m,) and dist.dtype == torch.float32 and index.dtype == torch.int32
    assert not dist.requires_grad
    return dist.cpu().numpy(), index.cpu().numpy()


def _check(got, query, target, expected, what):
    dist, index = got
    r_dist, r_index, r_best, flag = expected
    keep = ~flag
    none = ~np.isfinite(r_dist)
    assert np.array_equal(np.isinf(dist)[keep], none[keep]), (what, int((np.isinf(dist) != none)[keep].sum()))
    assert np.array_equal(index == -1, np.isinf(dist)), what
    assert not np.isnan(dist).any() and (index >= -1).all() and (index < max(len(target), 1)).all(), what
    have = keep & ~none
    err = np.abs(dist[have].astype(np.float64) - r_dist[have])
    lim = 2.0 ** -23 * r_dist[have]
    print("%s: %d of %d found, %d flagged, max dist err / bound %.3g" %
          (what, int(have.sum()), len(dist), int(flag.sum()), float((err / np.maximum(lim, 1e-300)).max(initial=0))))
    assert (err <= lim).all(), (what, float((err - lim).max()))
    d2 = ref.pair_d2(query, target, np.flatnonzero(have), index[have])
    assert (d2 <= r_best[have] * (1.0 + 1e-12)).all(), what


# ---- the restatement, on every size ------------------------------------------------------------
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "%s%d-%s%d" % c)
def test_nearest_matches_the_float64_restatement(case):
    query, target = ref.case_clouds(case)
    _check(_nearest(query, target), query, target, ref.case_reference(case), str(case))


# ---- known answers on integer coordinates: every d2 is exact --------------------------------------
def _lattice(n=6, step=4):
    g = np.arange(n) * step
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) + np.float32(300.0)


@pytest.mark.parametrize("cell", (None, 3.0, 20.0, 64.0))
def test_known_answers(cell):
    lat = _lattice()
    # a query on a target point: 0.0 and that index
    dist, index = _nearest(lat[::7], lat, 20.0, cell)
    assert (dist == 0.0).all() and np.array_equal(index, np.arange(len(lat))[::7])
    # two and four targets equidistant from a query, in different cells, the lowest index last in cell order
    c = np.array([320.0, 320.0, 320.0], np.float32)
    two = np.stack([c + [7, 0, 0], c - [7, 0, 0]]).astype(np.float32)
    dist, index = _nearest([c], two, 20.0, cell)
    assert dist[0] == 7.0 and index[0] == 0
    four = np.stack([c + [0, 0, 9], c + [0, 9, 0], c - [9, 0, 0], c - [0, 0, 9], c + [0, 0, 11]]).astype(np.float32)
    dist, index = _nearest([c], four, 20.0, cell)
    assert dist[0] == 9.0 and index[0] == 0
    dist, index = _nearest([c], four[::-1].copy(), 20.0, cell)
    assert dist[0] == 9.0 and index[0] == 1
    # 3-4-5: an exact non-axis distance; duplicated target points: the lowest index
    dup = np.stack([c + [30, 0, 0], c + [3, 4, 0], c + [0, 0, 12], c + [3, 4, 0], c + [3, 4, 0]]).astype(np.float32)
    dist, index = _nearest([c], dup, 20.0, cell)
    assert dist[0] == 5.0 and index[0] == 1
    # a target at exactly max_dist is found, one lattice step further is not
    far = np.stack([c + [0, 20, 0], c + [21, 0, 0], c + [12, 16, 1]]).astype(np.float32)
    dist, index = _nearest([c], far, 20.0, cell)
    assert dist[0] == 20.0 and index[0] == 0
    dist, index = _nearest([c], far[1:], 20.0, cell)
    assert dist[0] == INF and index[0] == -1
    dist, index = _nearest([c], [c + [12, 16, 0]], 20.0, cell)
    assert dist[0] == 20.0 and index[0] == 0


# ---- the result does not depend on the grid --------------------------------------------------------
def test_grid_independence():
    from mvs_amd import cloud_eval
    rng = np.random.default_rng(7)
    # coordinates that are multiples of 2.5: with cell 2.5 every point lies on a cell face; exact ties abound
    target = (rng.integers(0, 40, (4000, 3)) * 2.5 + ref.OFFSET).astype(np.float32)
    query = np.concatenate([(rng.integers(-4, 44, (450, 3)) * 2.5 + ref.OFFSET).astype(np.float32),
                            ref.box(150, 9)])
    expected = ref.nearest(query, target, MAX_DIST)
    assert not expected[3].any()
    q, t = _dev(query), _dev(target)
    first = None
    for cell in (None, MAX_DIST, 0.32, 500.0, 2.5, 7.3):      # R = 1; R = 63; the whole cloud one cell; faces; odd
        idx = cloud_eval.CloudIndex(t, MAX_DIST, cell)
        if cell == MAX_DIST:
            assert math.ceil(MAX_DIST / idx.cell) == 1
        if cell == 500.0:
            assert idx.dims == (1, 1, 1)
        if cell == 0.32:
            assert math.ceil(MAX_DIST / idx.cell) == 63
        got = idx.nearest(q)
        if first is None:
            first = got
            _check((got[0].cpu().numpy(), got[1].cpu().numpy()), query, target, expected, "lattice")
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), cell


# ---- structure ---------------------------------------------------------------------------------------
def test_crowded_cells_and_empty_cells():
    rng = np.random.default_rng(11)
    # 300 and 1100 points inside one cell each (several staging passes, the last one partial), far apart: most
    # cells are empty
    a = rng.uniform(0.0, 3.9, (300, 3)) + [300.0, 300.0, 300.0]
    b = rng.uniform(0.0, 3.9, (1100, 3)) + [348.0, 312.0, 300.0]
    target = np.concatenate([a, b]).astype(np.float32)
    query = np.concatenate([a[:40] + 0.3, b[-70:] - 0.2, rng.uniform(290.0, 360.0, (90, 3))]).astype(np.float32)
    expected = ref.nearest(query, target, MAX_DIST)
    assert not expected[3].any()
    for cell in (4.0, None):
        _check(_nearest(query, target, MAX_DIST, cell), query, target, expected, "crowded cell %s" % cell)
    # the nearest point of the last, partial pass: each query sits on a target of the tail of the big cell
    dist, index = _nearest(target[-5:], target, MAX_DIST, 4.0)
    assert (dist == 0.0).all() and np.array_equal(index, np.arange(len(target))[-5:])


def test_neighbour_several_rings_away_and_zero_extent():
    target = np.array([[300, 300, 300], [311, 300, 300], [300, 317, 300]], np.float32)
    query = np.array([[306, 300, 300], [300, 309, 301], [301, 301, 318.5]], np.float32)
    expected = ref.nearest(query, target, MAX_DIST)
    for cell in (1.0, 0.5, None):
        got = _nearest(query, target, MAX_DIST, cell)
        _check(got, query, target, expected, "rings %s" % cell)
        assert np.array_equal(got[1], [1, 2, 0]) and got[0][0] == 5.0
    # all targets identical: a grid of zero extent, one cell
    same = np.tile(np.array([[310.5, 290.25, 305.0]], np.float32), (700, 1))
    query = np.array([[310.5, 290.25, 305.0], [313.5, 294.25, 305.0], [310.5, 290.25, 326.0]], np.float32)
    dist, index = _nearest(query, same)
    assert np.array_equal(dist, np.array([0.0, 5.0, INF], np.float32)) and np.array_equal(index, [0, 0, -1])


def test_queries_outside_the_box():
    target = ref.box(1000, 3)
    rng = np.random.default_rng(13)
    lo, hi = target.min(0), target.max(0)
    # within max_dist of the box on every side, and beyond it
    shell = np.concatenate([rng.uniform(lo - 15.0, hi + 15.0, (600, 3)),
                            np.stack([lo - [19.0, 0, 0], hi + [0, 19.0, 0], lo - 12.0, hi + 11.0])]).astype(np.float32)
    expected = ref.nearest(shell, target, MAX_DIST)
    assert not expected[3].any() and np.isfinite(expected[0]).sum() > 300
    for cell in (None, 6.0, MAX_DIST):
        _check(_nearest(shell, target, MAX_DIST, cell), shell, target, expected, "shell %s" % cell)
    away = np.concatenate([rng.uniform(hi + 21.0, hi + 500.0, (100, 3)), rng.uniform(lo - 1e6, lo - 21.0, (100, 3)),
                           [[1e30, 0, 0], [-3e38, 3e38, 3e38]]]).astype(np.float32)
    for cell in (None, 0.5):
        dist, index = _nearest(away, target, MAX_DIST, cell)
        assert np.isinf(dist).all() and (index == -1).all()


def test_non_finite_coordinates_and_empty_clouds():
    from mvs_amd import cloud_eval
    target, query = np.array(ref.sheet(1000, 4)), np.array(ref.sheet(1000, 5))
    bad_t, bad_q = np.arange(0, 1000, 7), np.arange(3, 1000, 11)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        target[bad_t[k::3], k] = v
        query[bad_q[k::3], (k + 1) % 3] = v
    expected = ref.nearest(query, target, MAX_DIST)
    assert not expected[3].any()
    got = _nearest(query, target)
    _check(got, query, target, expected, "non-finite")
    assert not np.isin(got[1], bad_t).any()                       # never returned
    assert np.isinf(got[0][bad_q]).all() and (got[1][bad_q] == -1).all()
    # only non-finite targets; G = 0; M = 0
    for t in (np.full((5, 3), np.nan, np.float32), np.zeros((0, 3), np.float32)):
        dist, index = _nearest(query[:70], t)
        assert np.isinf(dist).all() and (dist > 0).all() and (index == -1).all()
    dist, index = _nearest(np.zeros((0, 3), np.float32), target)
    assert dist.shape == index.shape == (0,)
    idx = cloud_eval.CloudIndex(torch.zeros((0, 3), device=DEV), MAX_DIST)
    assert idx.n_points == 0 and idx.n_finite == 0 and idx.nearest(torch.zeros((0, 3), device=DEV))[0].shape == (0,)


# ---- repeat and stream -----------------------------------------------------------------------------
def test_repeat_side_stream_and_every_output_written():
    from mvs_amd import _lib, cloud_eval
    case = ("sheet", 5000, "sheet", 5000)
    query, target = (_dev(a) for a in ref.case_clouds(case))
    idx = cloud_eval.CloudIndex(target, MAX_DIST)
    first = idx.nearest(query)
    again = idx.nearest(query)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = cloud_eval.CloudIndex(target, MAX_DIST).nearest(query)
    side.synchronize()
    assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    # through the C entry into buffers pre-filled with garbage: every element is written
    order = torch.sort(cloud_eval.cell_keys_op(query, *idx._grid()), stable=True)[1].to(torch.int32)
    dist = torch.full((5000,), float("nan"), device=DEV)
    index = torch.full((5000,), -77, device=DEV, dtype=torch.int32)
    lib = _lib.load()
    st = lib.mvs_cloud_nearest(_lib.ptr(query), _lib.ptr(order), 5000, _lib.ptr(idx._targets), _lib.ptr(idx._index),
                               5000, _lib.ptr(idx._cell_start), *idx._grid(), MAX_DIST, _lib.ptr(dist),
                               _lib.ptr(index), _lib.stream_handle(DEV))
    assert st == 0
    assert torch.equal(dist, first[0]) and torch.equal(index, first[1])
    # the cell table likewise
    ncells = idx.dims[0] * idx.dims[1] * idx.dims[2]
    keys = torch.sort(cloud_eval.cell_keys_op(target, *idx._grid()))[0]
    table = torch.full((ncells + 1,), -5, device=DEV, dtype=torch.int32)
    assert lib.mvs_cloud_cell_ranges(_lib.ptr(keys), 5000, ncells, _lib.ptr(table), _lib.stream_handle(DEV)) == 0
    assert torch.equal(table, idx._cell_start) and int(table[0]) == 0 and int(table[-1]) == 5000
    counts = torch.bincount(keys.long(), minlength=ncells + 1)[:ncells]
    assert torch.equal(table[1:] - table[:-1], counts.to(torch.int32))


# ---- evaluate_cloud ----------------------------------------------------------------------------------
def _same(got, want, what):
    for key in ("accuracy", "completeness", "overall"):
        if math.isnan(want[key]):
            assert math.isnan(got[key]), (what, key)
        else:
            assert abs(got[key] - want[key]) <= 1e-6 * abs(want[key]), (what, key, got[key], want[key])
    for key in ("accuracy_median", "completeness_median"):
        assert got[key] == want[key] or (math.isnan(got[key]) and math.isnan(want[key])), (what, key, got[key])
    for key in ("n_pred_inliers", "n_gt_inliers"):
        assert got[key] == want[key] and isinstance(got[key], int), (what, key, got[key], want[key])
    for key in ("precision", "recall", "fscore"):
        assert sorted(got[key]) == sorted(want[key]), (what, key)
        for tau in want[key]:
            assert abs(got[key][tau] - want[key][tau]) <= 1e-12, (what, key, tau, got[key][tau], want[key][tau])


def test_evaluate_cloud():
    from mvs_amd import cloud_eval
    pred, gt = np.array(ref.sheet(5000, 1)), np.array(ref.sheet(1000, 2))
    pred[:300, 2] += np.float32(60.0)                 # outliers beyond max_dist
    pred[5::97, 1] = np.nan
    taus = (0.5, 2.0, 20.0)
    want, flagged = ref.evaluate(pred, gt, MAX_DIST, taus)
    assert not flagged and 0 < want["n_pred_inliers"] < 4700 and want["n_gt_inliers"] == 1000
    got = cloud_eval.evaluate_cloud(_dev(pred), _dev(gt), MAX_DIST, taus)
    assert all(isinstance(got[k], float) for k in ("accuracy", "completeness", "overall", "accuracy_median"))
    _same(got, want, "sheets")
    # a cloud against itself
    got = cloud_eval.evaluate_cloud(_dev(gt), _dev(gt), MAX_DIST, (1.0,))
    assert got["accuracy"] == got["completeness"] == got["overall"] == got["accuracy_median"] == 0.0
    assert got["n_pred_inliers"] == got["n_gt_inliers"] == 1000
    assert got["precision"][1.0] == got["recall"][1.0] == got["fscore"][1.0] == 1.0
    # a sparse lattice shifted by a known lattice vector: 3-4-12 -> 13 everywhere
    g = np.arange(5) * 40
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) + np.float32(200.0)
    got = cloud_eval.evaluate_cloud(_dev(lat + np.float32([3, 4, 12])), _dev(lat), MAX_DIST, (13.0, 13.5))
    assert got["accuracy"] == got["completeness"] == got["accuracy_median"] == got["completeness_median"] == 13.0
    assert got["n_pred_inliers"] == got["n_gt_inliers"] == 125
    assert got["precision"][13.0] == 0.0 and got["fscore"][13.0] == 0.0 and got["fscore"][13.5] == 1.0
    # disjoint clouds farther than max_dist apart
    got = cloud_eval.evaluate_cloud(_dev(lat), _dev(lat + np.float32(1000.0)), MAX_DIST, (5.0,))
    assert math.isnan(got["accuracy"]) and math.isnan(got["completeness"]) and math.isnan(got["overall"])
    assert math.isnan(got["accuracy_median"]) and got["n_pred_inliers"] == got["n_gt_inliers"] == 0
    assert got["precision"][5.0] == got["recall"][5.0] == got["fscore"][5.0] == 0.0


def test_index_reused_for_two_query_clouds():
    from mvs_amd import cloud_eval
    target = _dev(ref.sheet(5000, 2))
    idx = cloud_eval.CloudIndex(target, MAX_DIST)
    for query in (_dev(ref.sheet(1000, 1)), _dev(ref.box(1000, 1))):
        one = cloud_eval.nearest_distance(query, target, MAX_DIST)
        got = idx.nearest(query)
        assert torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
