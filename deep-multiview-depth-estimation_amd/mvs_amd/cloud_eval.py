"""Cloud evaluation: how far a reconstructed point cloud lies from a ground-truth cloud, the step after
mvs_amd.fusion (the reference has none).

  CloudIndex(points, max_dist, cell=None)         a uniform grid over a cloud, built once
  CloudIndex.nearest(query) -> (dist, index)      per query point the nearest indexed point within max_dist
  nearest_distance(query, target, max_dist, cell=None) -> (dist, index)   the same in one call
  evaluate_cloud(pred, gt, max_dist=20.0, thresholds=()) -> dict          accuracy, completeness, precision / recall

The definition (include/fusion/mvs_cloud_eval.h) does not depend on the grid: in float64 on the widened fp32
coordinates, d2 = dx dx + dy dy + dz dz; a target with a non-finite coordinate is never a candidate, nor is one with
d2 > max_dist^2; ``index`` is the lowest target index that reaches the minimum exactly, ``dist`` the square root of
the minimum rounded once to fp32; a query with no candidate, or with a non-finite coordinate, gets +inf and -1.

The search runs on the HIP kernels of csrc/cloud_nn.hip: no atomics, every output written once, two calls are
torch.equal.  Sorting keys and gathering points into cell order are torch ops.  Device tensors only: there is no CPU
fallback.  Nothing here is differentiable: inputs are detached and the ops register no autograd.  Calling these
functions is the opt-in: no environment switch selects them and MVSNet.forward does not route to them.

The ops (namespace ``mvs_cloud``), each with a fake kernel:
  mvs_cloud::cell_keys(points, ox, oy, oz, cell, nx, ny, nz) -> keys int32 [n]
  mvs_cloud::cell_ranges(sorted_keys, ncells) -> cell_start int32 [ncells + 1]
  mvs_cloud::nearest(query, query_order, targets, target_index, cell_start, ox, oy, oz, cell, nx, ny, nz, max_dist)
      -> (dist fp32 [m], index int32 [m])"""
import math
from typing import Tuple

import torch

from . import _lib
from .ops import _require_gpu

_F32 = torch.float32
# the default cell edge aims at this many points per occupied cell of a surface-like cloud (DESIGN.md §3.11 has the
# sweep it was chosen from)
POINTS_PER_CELL = 16.0


def _check_cloud(points, name):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s must be a tensor [n, 3], got %s" % (name, tuple(getattr(points, "shape", ())) or
                                                                 type(points).__name__))
    if points.dtype != _F32:
        raise ValueError("%s must be fp32, got %s" % (name, points.dtype))


def _cloud(points, name):
    """points as detached contiguous fp32 [n, 3] on its (HIP) device; shape and dtype are checked first."""
    _check_cloud(points, name)
    _require_gpu(points, name)
    return points.detach().contiguous()


def _positive(value, name):
    value = float(value)
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError("%s must be finite and > 0, got %r" % (name, value))
    return value


def _check_rings(max_dist, cell):
    if math.ceil(max_dist / cell) > _lib.CLOUD_MAX_RINGS:
        raise ValueError("cell %g puts max_dist %g more than %d rings away (the ring limit); use a cell of at least %g"
                         % (cell, max_dist, _lib.CLOUD_MAX_RINGS, max_dist / _lib.CLOUD_MAX_RINGS))


def grid_dims(lo, hi, cell):
    """(nx, ny, nz) of the grid of edge ``cell`` over the box lo .. hi (float64 triples): floor(extent / cell) + 1 per
    axis, the arithmetic by which the kernel assigns cells, so the far corner lies in the last cell."""
    return tuple(int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi))


def choose_grid(lo, hi, count, max_dist, cell=None):
    """(cell, (nx, ny, nz)) for ``count`` finite points in the box lo .. hi.  An explicit ``cell`` is taken as it is,
    and ValueError names the limit it breaks (2^27 cells, 64 rings).  The default aims at POINTS_PER_CELL points per
    occupied cell for points on a surface (cell^2 = POINTS_PER_CELL * the product of the two largest extents /
    count), is at least max_dist / 64 (the ring limit), and grows by 2^(1/3) until the grid fits the cell limit."""
    max_dist = _positive(max_dist, "max_dist")
    if cell is not None:
        cell = _positive(cell, "cell")
        _check_rings(max_dist, cell)
        dims = grid_dims(lo, hi, cell)
        if dims[0] * dims[1] * dims[2] > _lib.CLOUD_MAX_CELLS:
            raise ValueError("cell %g makes a grid of %d x %d x %d cells, more than 2^27 (the cell limit)"
                             % ((cell,) + dims))
        return cell, dims
    ext = sorted(h - l for l, h in zip(lo, hi))
    cell = max(math.sqrt(POINTS_PER_CELL * ext[1] * ext[2] / max(count, 1)), max_dist / _lib.CLOUD_MAX_RINGS)
    while True:
        dims = grid_dims(lo, hi, cell)
        if dims[0] * dims[1] * dims[2] <= _lib.CLOUD_MAX_CELLS:
            return cell, dims
        cell *= 2.0 ** (1.0 / 3.0)


# ----------------------------------------------------------------------------------------------
# the ops
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("mvs_cloud::cell_keys", mutates_args=())
def cell_keys_op(points: torch.Tensor, ox: float, oy: float, oz: float, cell: float, nx: int, ny: int,
                 nz: int) -> torch.Tensor:
    """keys int32 [n] of points fp32 [n, 3]: the linear cell (cz ny + cy) nx + cx with c = floor((p - origin) / cell)
    in float64 clamped to the grid, nx ny nz for a point with a non-finite coordinate.  (mvs_cloud_cell_keys)"""
    points = _cloud(points, "points")
    lib = _lib.load()
    keys = torch.empty((points.shape[0],), device=points.device, dtype=torch.int32)
    st = lib.mvs_cloud_cell_keys(_lib.ptr(points), points.shape[0], ox, oy, oz, cell, nx, ny, nz, _lib.ptr(keys),
                                 _lib.stream_handle(points.device))
    _lib.check(st, "mvs_cloud_cell_keys")
    return keys


@cell_keys_op.register_fake
def _(points, ox, oy, oz, cell, nx, ny, nz):
    return points.new_empty((points.shape[0],), dtype=torch.int32)


@torch.library.custom_op("mvs_cloud::cell_ranges", mutates_args=())
def cell_ranges_op(sorted_keys: torch.Tensor, ncells: int) -> torch.Tensor:
    """cell_start int32 [ncells + 1] of ascending keys int32 [n] in [0, ncells]: cell k holds the sorted positions
    cell_start[k] .. cell_start[k + 1] - 1.  (mvs_cloud_cell_ranges)"""
    _require_gpu(sorted_keys, "sorted_keys")
    if sorted_keys.dim() != 1 or sorted_keys.dtype != torch.int32:
        raise ValueError("sorted_keys must be int32 [n], got %s %s" % (sorted_keys.dtype, tuple(sorted_keys.shape)))
    lib = _lib.load()
    keys = sorted_keys.contiguous()
    start = torch.empty((max(ncells, 0) + 1,), device=keys.device, dtype=torch.int32)
    st = lib.mvs_cloud_cell_ranges(_lib.ptr(keys), keys.shape[0], ncells, _lib.ptr(start),
                                   _lib.stream_handle(keys.device))
    _lib.check(st, "mvs_cloud_cell_ranges")
    return start


@cell_ranges_op.register_fake
def _(sorted_keys, ncells):
    return sorted_keys.new_empty((ncells + 1,), dtype=torch.int32)


@torch.library.custom_op("mvs_cloud::nearest", mutates_args=())
def nearest_op(query: torch.Tensor, query_order: torch.Tensor, targets: torch.Tensor, target_index: torch.Tensor,
               cell_start: torch.Tensor, ox: float, oy: float, oz: float, cell: float, nx: int, ny: int, nz: int,
               max_dist: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist fp32 [m], index int32 [m]) of query fp32 [m, 3] with query_order int32 [m] (the queries in cell order),
    targets fp32 [g, 3] in cell order, target_index int32 [g] (their original indices) and the cell_start table of the
    same grid, all on one device.  One launch on the current stream.  (mvs_cloud_nearest)"""
    query, targets = _cloud(query, "query"), _cloud(targets, "targets")
    m, g, dev = query.shape[0], targets.shape[0], query.device
    for t, n, name in ((query_order, m, "query_order"), (target_index, g, "target_index"),
                       (cell_start, nx * ny * nz + 1, "cell_start")):
        if tuple(t.shape) != (n,) or t.dtype != torch.int32 or t.device != dev:
            raise ValueError("%s must be int32 [%d] on the queries' device, got %s %s on %s"
                             % (name, n, t.dtype, tuple(t.shape), t.device))
    if targets.device != dev:
        raise ValueError("targets must be on the queries' device")
    lib = _lib.load()
    dist = torch.empty((m,), device=dev, dtype=_F32)
    index = torch.empty((m,), device=dev, dtype=torch.int32)
    st = lib.mvs_cloud_nearest(_lib.ptr(query), _lib.ptr(query_order.contiguous()), m, _lib.ptr(targets),
                               _lib.ptr(target_index.contiguous()), g, _lib.ptr(cell_start.contiguous()), ox, oy, oz,
                               cell, nx, ny, nz, max_dist, _lib.ptr(dist), _lib.ptr(index), _lib.stream_handle(dev))
    _lib.check(st, "mvs_cloud_nearest")
    return dist, index


@nearest_op.register_fake
def _(query, query_order, targets, target_index, cell_start, ox, oy, oz, cell, nx, ny, nz, max_dist):
    m = query.shape[0]
    return query.new_empty((m,), dtype=_F32), query.new_empty((m,), dtype=torch.int32)


# ----------------------------------------------------------------------------------------------
# the index
# ----------------------------------------------------------------------------------------------
class CloudIndex:
    """A uniform grid over ``points`` fp32 [G, 3] on the device for nearest-neighbour queries within ``max_dist``.

    Building it synchronises with the host once: the bounding box of the finite points and their count come back to
    size the cell table.  ``cell`` is the edge of a grid cell; None picks one (choose_grid) that keeps the grid
    within 2^27 cells and max_dist within 64 rings of cells, an explicit value that breaks either limit raises
    ValueError.  The results do not depend on it.  Attributes: cell, dims (nx, ny, nz), origin, n_points, n_finite."""

    def __init__(self, points, max_dist, cell=None):
        _check_cloud(points, "points")                    # (argument errors before the device is asked for)
        self.max_dist = _positive(max_dist, "max_dist")
        if cell is not None:
            _check_rings(self.max_dist, _positive(cell, "cell"))
        points = _cloud(points, "points")
        self.device, self.n_points = points.device, points.shape[0]
        self.n_finite, self.cell, self.dims, self.origin = 0, None, None, None
        if self.n_points == 0:
            return
        finite = torch.isfinite(points).all(dim=1, keepdim=True)
        wide = points.to(torch.float64)
        box = torch.cat([torch.where(finite, wide, math.inf).amin(0), torch.where(finite, wide, -math.inf).amax(0),
                         finite.sum().to(torch.float64).reshape(1)]).cpu().tolist()     # the one synchronisation
        self.n_finite = int(box[6])
        if self.n_finite == 0:
            return
        lo, hi = box[0:3], box[3:6]
        self.cell, self.dims = choose_grid(lo, hi, self.n_finite, self.max_dist, cell)
        self.origin = tuple(lo)
        keys = cell_keys_op(points, *self._grid())
        keys, order = torch.sort(keys, stable=True)
        self._index = order.to(torch.int32)
        self._targets = points.index_select(0, order)
        self._cell_start = cell_ranges_op(keys, self.dims[0] * self.dims[1] * self.dims[2])

    def _grid(self):
        return self.origin + (self.cell,) + self.dims

    def nearest(self, query):
        """(dist fp32 [M], index int32 [M]) for query fp32 [M, 3] on the index's device: the distance to the nearest
        indexed point within max_dist and its index in ``points`` (the lowest on an exact tie); +inf and -1 where
        there is none or the query has a non-finite coordinate.  No host synchronisation."""
        query = _cloud(query, "query")
        if query.device != self.device:
            raise ValueError("query is on %s, the index on %s" % (query.device, self.device))
        m = query.shape[0]
        if m == 0 or self.n_finite == 0:               # nothing to search: no launch
            return (torch.full((m,), math.inf, device=self.device, dtype=_F32),
                    torch.full((m,), -1, device=self.device, dtype=torch.int32))
        order = torch.sort(cell_keys_op(query, *self._grid()), stable=True)[1].to(torch.int32)
        return nearest_op(query, order, self._targets, self._index, self._cell_start, *self._grid(), self.max_dist)


def nearest_distance(query, target, max_dist, cell=None):
    """(dist fp32 [M], index int32 [M]): CloudIndex(target, max_dist, cell).nearest(query)."""
    _check_cloud(query, "query")
    return CloudIndex(target, max_dist, cell).nearest(query)


def _one_way(dist, points, taus):
    """(mean, median, inliers, [share of the finite-coordinate points with dist < tau]) as device float64 scalars."""
    inl = torch.isfinite(dist)
    d = dist.to(torch.float64)
    n_in = inl.sum()
    nan = torch.full((), math.nan, device=dist.device, dtype=torch.float64)
    mean = torch.where(n_in > 0, torch.where(inl, d, 0.0).sum() / n_in, nan)
    # the lower median of the inliers: the (n_in - 1) // 2-th of the ascending distances (+inf sorts last)
    if dist.numel():
        pick = ((n_in - 1).clamp(min=0) // 2).reshape(1)
        median = torch.where(n_in > 0, torch.sort(d)[0].gather(0, pick)[0], nan)
    else:
        median = nan
    n_pts = torch.isfinite(points).all(dim=1).sum()
    shares = [torch.where(n_pts > 0, (d < tau).sum().to(torch.float64) / n_pts, nan) for tau in taus]
    return [mean, median, n_in.to(torch.float64)] + shares


def evaluate_cloud(pred, gt, max_dist=20.0, thresholds=()):
    """A dict of Python numbers for pred fp32 [M, 3] against gt fp32 [G, 3], both on the device:

      accuracy, accuracy_median          mean and (lower) median of the pred -> gt distances that are finite, that is
                                         within max_dist: DTU's outlier rule excludes what lies beyond
      completeness, completeness_median  the same for gt -> pred
      overall                            (accuracy + completeness) / 2
      n_pred_inliers, n_gt_inliers       how many distances those means are over
      precision, recall, fscore          per tau in ``thresholds``, as dicts keyed by tau: the share of the pred (gt)
                                         points with finite coordinates whose distance is < tau, and
                                         2 p r / (p + r), 0 when both are 0 (Tanks and Temples' measure)

    Every tau must satisfy 0 < tau <= max_dist (a distance beyond max_dist is not known).  A mean over no terms is
    nan.  The reductions are float64 torch ops on the device; one copy brings the numbers to the host.

    This is the distance part of DTU's protocol only.  DTU's evaluation also restricts both clouds to its
    observation mask and cuts off what lies below its ground plane, and first thins the reconstruction to one point
    per 0.2 mm; none of that is done here, so figures from raw clouds are not comparable with published DTU tables."""
    max_dist = _positive(max_dist, "max_dist")
    taus = [float(t) for t in thresholds]
    for tau in taus:
        if not (0.0 < tau <= max_dist):
            raise ValueError("threshold %r must satisfy 0 < tau <= max_dist = %g" % (tau, max_dist))
    _check_cloud(pred, "pred")
    _check_cloud(gt, "gt")
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    d_pred = CloudIndex(gt, max_dist).nearest(pred)[0]
    d_gt = CloudIndex(pred, max_dist).nearest(gt)[0]
    vals = torch.stack(_one_way(d_pred, pred, taus) + _one_way(d_gt, gt, taus)).cpu().tolist()
    k = 3 + len(taus)
    acc, comp = vals[0], vals[k]
    out = {"accuracy": acc, "completeness": comp, "accuracy_median": vals[1], "completeness_median": vals[k + 1],
           "overall": 0.5 * (acc + comp), "n_pred_inliers": int(vals[2]), "n_gt_inliers": int(vals[k + 2]),
           "precision": {}, "recall": {}, "fscore": {}}
    for i, tau in enumerate(taus):
        p, r = vals[3 + i], vals[k + 3 + i]
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 0.0 if p == 0.0 and r == 0.0 else 2.0 * p * r / (p + r)
    return out
