"""Depth-map filtering and fusion: what an MVSNet pipeline does with the depth maps of a scan's N views.  The
reference stops at the depth maps; this is new ground with an API of its own, in the style of mvs_amd.loss.

  photometric_confidence(prob_volume, depth, d_batch) -> [B, 1, h, w]
      the probability mass of the four hypothesis planes around the estimated depth (MVSNet's confidence)
  geometric_consistency(depth, K, R, T, pairs, px_thresh=1.0, rel_thresh=0.01) -> (n_consistent, depth_avg)
      per pixel of each view, the number of its source views whose depth map agrees with it after a round trip
      (within px_thresh pixels and rel_thresh of the depth), and the average of the agreeing depths
  filter_depth(depth, confidence, K, R, T, pairs, ...) -> (mask, depth_avg)
  point_cloud(depth, mask, K, R, T, colors=None) -> points [M, 3] (, colors [M, 3])
  fused_point_cloud(depth, mask, K, R, T, pairs, colors=None, ...) -> points [M, 3] (, colors [M, 3]) (, n_merged [M])
      the cloud with each surface point emitted once across the views: views go in index order, a kept pixel that
      no earlier view has absorbed is emitted and absorbs the pixels of its sources that agree with it
  write_ply(path, points, colors=None)
  read_ply(path) -> (points, colors or None)

Everything per pixel runs on the HIP kernels of csrc/depth_filter.hip and csrc/depth_fuse.hip
(include/fusion/mvs_depth_filter.h, mvs_view_fusion.h): one thread per output pixel, the geometry in float64, every output written once, no atomics and no host
synchronisation -- instead of a device-to-host copy per view and a numpy loop over the pairs.  Device tensors only:
there is no CPU fallback.  Calling these functions is the opt-in: no environment switch selects them, MVSNet.forward
does not route to them (MVSNet.forward_with_confidence does, for the confidence).

Cameras follow the package's convention: x_cam = R x_world + T, K at the maps' resolution, integer pixel indices.  A
depth is valid when it is > 0.

The ops live in the namespace ``mvs_fusion`` (the ``mvs`` namespace is the drop-in surface and stays as it is); none
registers autograd, and the functions above hand them detached tensors, so their results do not require grad:
  mvs_fusion::photometric_confidence(prob_volume, depth, d_batch) -> conf
  mvs_fusion::view_pair_matrices(K, R, T, pairs) -> matrices [N, S, 24] float64
  mvs_fusion::geometric_consistency(depth, pairs, matrices, px_thresh, rel_thresh) -> (n_consistent, depth_avg)
  mvs_fusion::backproject(depth, K, R, T) -> xyz [N, h, w, 3]
  mvs_fusion::fuse_views(depth, mask, colors?, K, R, T, pairs, matrices, px_thresh, rel_thresh)
      -> (emitted bool [N, h, w], n_merged int32 [N, h, w], xyz [N, h, w, 3], rgb [N, h, w, 3] or empty)"""
import ctypes
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _require_gpu

_F32 = torch.float32


def _depth_maps(depth, what):
    """depth as contiguous fp32 [N, 1, h, w] on its (HIP) device."""
    _require_gpu(depth, "depth")
    if depth.dim() != 4 or depth.shape[1] != 1 or depth.dtype != _F32:
        raise ValueError("%s: depth must be fp32 [N, 1, h, w], got %s %s" % (what, depth.dtype, tuple(depth.shape)))
    return depth.contiguous()


def _view_cams(K, R, T, device, n, what):
    """K, R [n, 3, 3] and T [n, 3] as contiguous fp32 on ``device`` (host or device tensors, moved as ops._cams
    moves them)."""
    K = K.to(device=device, dtype=_F32).reshape(-1, 3, 3).contiguous()
    R = R.to(device=device, dtype=_F32).reshape(-1, 3, 3).contiguous()
    T = T.to(device=device, dtype=_F32).reshape(-1, 3).contiguous()
    if not (K.shape[0] == R.shape[0] == T.shape[0] == n):
        raise ValueError("%s: %d depth maps, but %d / %d / %d cameras in K / R / T"
                         % (what, n, K.shape[0], R.shape[0], T.shape[0]))
    return K, R, T


def pair_table(pairs, n_views):
    """``pairs`` as a CPU int32 tensor [n_views, S], S >= 1: a nested list (ragged rows are padded with -1) or an
    integer tensor with -1 padding.  ValueError for an index outside [-1, n_views), for more or fewer rows than
    views and for more than 64 slots."""
    if isinstance(pairs, torch.Tensor):
        if pairs.dim() != 2 or pairs.dtype.is_floating_point or pairs.dtype == torch.bool:
            raise ValueError("pairs must be an integer tensor [N, S], got %s %s" % (pairs.dtype, tuple(pairs.shape)))
        table = pairs.detach().to(device="cpu", dtype=torch.int64)
        if table.shape[1] == 0:
            table = table.new_full((table.shape[0], 1), -1)
    else:
        rows = [[int(v) for v in row] for row in pairs]
        width = max([len(r) for r in rows] + [1])
        table = torch.tensor([r + [-1] * (width - len(r)) for r in rows], dtype=torch.int64).reshape(len(rows), width)
    if table.shape[0] != n_views:
        raise ValueError("pairs holds %d rows for %d views" % (table.shape[0], n_views))
    if table.shape[1] > _lib.FILTER_MAX_SLOTS:
        raise ValueError("pairs holds %d source slots per view, at most %d" % (table.shape[1], _lib.FILTER_MAX_SLOTS))
    if table.numel() and (int(table.min()) < -1 or int(table.max()) >= n_views):
        raise ValueError("pairs names a view outside [-1, %d)" % n_views)
    return table.to(torch.int32).contiguous()


# ----------------------------------------------------------------------------------------------
# mvs_fusion::photometric_confidence
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("mvs_fusion::photometric_confidence", mutates_args=())
def photometric_confidence_op(prob_volume: torch.Tensor, depth: torch.Tensor,
                              d_batch: torch.Tensor) -> torch.Tensor:
    """conf [B, 1, h, w] of prob_volume [B, 1, D, h, w], depth [B, 1, h, w] and the planes d_batch [B, D] (or [1, D],
    expanded as extract_depth_map expands it) that the depth was extracted with: with t = (depth - d_0) / (d_1 - d_0)
    in fp32 and k0 = floor(t) clamped to [0, D - 1], the sum of P_k over k = k0 - 1 .. k0 + 2 inside [0, D), added in
    ascending k.  A NaN depth gives 0.  (mvs_photometric_confidence_fwd)"""
    _require_gpu(prob_volume, "prob_volume")
    lib = _lib.load()
    if prob_volume.dim() != 5 or prob_volume.shape[1] != 1:
        raise ValueError("prob_volume must be [B, 1, D, h, w], got %s" % (tuple(prob_volume.shape),))
    prob = prob_volume.to(_F32).contiguous()
    b, _, d, h, w = prob.shape
    if tuple(depth.shape) != (b, 1, h, w):
        raise ValueError("depth must be [%d, 1, %d, %d], got %s" % (b, h, w, tuple(depth.shape)))
    if d < 2:
        raise ValueError("photometric_confidence: at least two depth planes expected, got %d" % d)
    dep = depth.to(device=prob.device, dtype=_F32).contiguous()
    db = d_batch.to(device=prob.device, dtype=_F32).reshape(-1, d)
    if db.shape[0] == 1 and b > 1:
        db = db.expand(b, d)
    if db.shape[0] != b:
        raise ValueError("d_batch must be [%d, %d] or [1, %d], got %s" % (b, d, d, tuple(d_batch.shape)))
    db = db.contiguous()
    conf = torch.empty((b, 1, h, w), device=prob.device, dtype=_F32)
    st = lib.mvs_photometric_confidence_fwd(_lib.ptr(prob), _lib.ptr(dep), _lib.ptr(db), b, d, h, w, _lib.ptr(conf),
                                            _lib.stream_handle(prob.device))
    _lib.check(st, "mvs_photometric_confidence_fwd")
    return conf


@photometric_confidence_op.register_fake
def _(prob_volume, depth, d_batch):
    b, _, d, h, w = prob_volume.shape
    return prob_volume.new_empty((b, 1, h, w), dtype=_F32)


def photometric_confidence(prob_volume, depth, d_batch):
    """conf fp32 [B, 1, h, w]: the probability mass of the four hypothesis planes around ``depth`` [B, 1, h, w] in
    prob_volume [B, 1, D, h, w], with d_batch [B, D] or [1, D] the planes the depth was extracted with (the op's
    docstring has the definition).  Values in [0, 1] up to rounding for a softmax volume; 0 for a NaN depth.  Not
    differentiable: the inputs are detached."""
    return photometric_confidence_op(prob_volume.detach(), depth.detach(), d_batch.detach())


# ----------------------------------------------------------------------------------------------
# mvs_fusion::view_pair_matrices, mvs_fusion::geometric_consistency
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("mvs_fusion::view_pair_matrices", mutates_args=())
def view_pair_matrices(K: torch.Tensor, R: torch.Tensor, T: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
    """matrices [N, S, 24] float64 of device cameras K, R [N, 3, 3], T [N, 3] (fp32) and pairs [N, S] int32 on the
    same device: per (view n, slot s) M = K_s R_s R_n^T K_n^-1, m = K_s (T_s - R_s R_n^T T_n) and the same pair for
    the way back, formed in float64; zeros for an empty slot (-1, or the view itself).  (mvs_view_pair_matrices)"""
    _require_gpu(K, "K")
    lib = _lib.load()
    if pairs.dim() != 2 or pairs.dtype != torch.int32 or pairs.device != K.device:
        raise ValueError("pairs must be int32 [N, S] on the cameras' device, got %s %s on %s"
                         % (pairs.dtype, tuple(pairs.shape), pairs.device))
    n, s = pairs.shape
    K, R, T = _view_cams(K, R, T, K.device, n, "view_pair_matrices")
    pairs = pairs.contiguous()
    if lib.mvs_view_pair_matrices_bytes(n, s) == 0:
        raise ValueError("view_pair_matrices: N >= 1 views and 1 <= S <= %d slots expected, got %d and %d"
                         % (_lib.FILTER_MAX_SLOTS, n, s))
    out = torch.empty((n, s, 24), device=K.device, dtype=torch.float64)
    st = lib.mvs_view_pair_matrices(_lib.ptr(K), _lib.ptr(R), _lib.ptr(T), _lib.ptr(pairs), n, s, _lib.ptr(out),
                                    _lib.stream_handle(K.device))
    _lib.check(st, "mvs_view_pair_matrices")
    return out


@view_pair_matrices.register_fake
def _(K, R, T, pairs):
    return K.new_empty((pairs.shape[0], pairs.shape[1], 24), dtype=torch.float64)


@torch.library.custom_op("mvs_fusion::geometric_consistency", mutates_args=())
def geometric_consistency_op(depth: torch.Tensor, pairs: torch.Tensor, matrices: torch.Tensor, px_thresh: float,
                             rel_thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(n_consistent int32, depth_avg fp32), both [N, 1, h, w], of depth fp32 [N, 1, h, w], pairs int32 [N, S] and
    the matrices view_pair_matrices formed for them, all on one device.  (mvs_geometric_consistency_fwd)"""
    depth = _depth_maps(depth, "geometric_consistency")
    lib = _lib.load()
    n, _, h, w = depth.shape
    if pairs.dim() != 2 or pairs.dtype != torch.int32 or pairs.device != depth.device or pairs.shape[0] != n:
        raise ValueError("pairs must be int32 [%d, S] on the depth maps' device, got %s %s on %s"
                         % (n, pairs.dtype, tuple(pairs.shape), pairs.device))
    s = pairs.shape[1]
    if tuple(matrices.shape) != (n, s, 24) or matrices.dtype != torch.float64 or matrices.device != depth.device:
        raise ValueError("matrices must be float64 [%d, %d, 24] on the depth maps' device, got %s %s on %s"
                         % (n, s, matrices.dtype, tuple(matrices.shape), matrices.device))
    for v, name in ((px_thresh, "px_thresh"), (rel_thresh, "rel_thresh")):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError("geometric_consistency: %s must be finite and > 0, got %r" % (name, v))
    pairs, matrices = pairs.contiguous(), matrices.contiguous()
    count = torch.empty((n, 1, h, w), device=depth.device, dtype=torch.int32)
    avg = torch.empty((n, 1, h, w), device=depth.device, dtype=_F32)
    st = lib.mvs_geometric_consistency_fwd(_lib.ptr(depth), _lib.ptr(pairs), _lib.ptr(matrices), n, s, h, w,
                                           float(px_thresh), float(rel_thresh), _lib.ptr(count), _lib.ptr(avg),
                                           _lib.stream_handle(depth.device))
    _lib.check(st, "mvs_geometric_consistency_fwd")
    return count, avg


@geometric_consistency_op.register_fake
def _(depth, pairs, matrices, px_thresh, rel_thresh):
    return depth.new_empty(depth.shape, dtype=torch.int32), depth.new_empty(depth.shape, dtype=_F32)


def geometric_consistency(depth, K, R, T, pairs, px_thresh=1.0, rel_thresh=0.01):
    """(n_consistent int32 [N, 1, h, w], depth_avg fp32 [N, 1, h, w]) of the N depth maps of a scan.

    depth [N, 1, h, w] fp32 on the device, each view's map in its own camera; K, R [N, 3, 3] and T [N, 3, 1] on host
    or device; pairs: per view the indices of its source views, a nested list (rows may differ in length) or a CPU
    integer tensor [N, S] padded with -1.  A slot that is -1 or names the view itself is empty; an index outside
    [-1, N) raises ValueError.

    Per pixel (x, y) of view n with depth d > 0 and per source s, in float64: the pixel is projected into s at depth
    d, the source's depth d_s is blended there from its four neighbours (all inside the map and > 0), that point is
    projected back into n, and the source is consistent when it lands within px_thresh pixels of (x, y) at a depth
    d_r with |d_r - d| < rel_thresh * d.  n_consistent counts the consistent sources; depth_avg = (d + the sum of
    their d_r) / (1 + n_consistent).  An invalid pixel gets 0 in both."""
    n = depth.shape[0] if isinstance(depth, torch.Tensor) and depth.dim() else 0
    table = pair_table(pairs, n)
    depth = _depth_maps(depth.detach(), "geometric_consistency")
    K, R, T = _view_cams(K.detach(), R.detach(), T.detach(), depth.device, n, "geometric_consistency")
    table = table.to(depth.device)
    matrices = view_pair_matrices(K, R, T, table)
    return geometric_consistency_op(depth, table, matrices, float(px_thresh), float(rel_thresh))


def filter_depth(depth, confidence, K, R, T, pairs, conf_thresh=0.8, min_consistent=2, px_thresh=1.0,
                 rel_thresh=0.01):
    """(mask bool [N, 1, h, w], depth_avg fp32 [N, 1, h, w]): the pixels of each view that survive both filters,
        mask = (depth > 0) & (confidence >= conf_thresh) & (n_consistent >= min_consistent),
    and geometric_consistency's averaged depths.  ``confidence`` [N, 1, h, w] (photometric_confidence of each view);
    None skips that term."""
    n_consistent, depth_avg = geometric_consistency(depth, K, R, T, pairs, px_thresh, rel_thresh)
    mask = (depth > 0) & (n_consistent >= int(min_consistent))
    if confidence is not None:
        if confidence.shape != depth.shape:
            raise ValueError("confidence must be %s, got %s" % (tuple(depth.shape), tuple(confidence.shape)))
        mask = mask & (confidence.to(depth.device) >= conf_thresh)
    return mask, depth_avg


# ----------------------------------------------------------------------------------------------
# mvs_fusion::backproject
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("mvs_fusion::backproject", mutates_args=())
def backproject_op(depth: torch.Tensor, K: torch.Tensor, R: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """xyz [N, h, w, 3] fp32, the world point of every pixel of depth fp32 [N, 1, h, w]:
    R_n^T (d K_n^-1 (x, y, 1)^T - T_n) in float64, rounded once; three zeros where d is not > 0.
    (mvs_backproject_fwd)"""
    depth = _depth_maps(depth, "backproject")
    lib = _lib.load()
    n, _, h, w = depth.shape
    K, R, T = _view_cams(K, R, T, depth.device, n, "backproject")
    xyz = torch.empty((n, h, w, 3), device=depth.device, dtype=_F32)
    st = lib.mvs_backproject_fwd(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(R), _lib.ptr(T), n, h, w, _lib.ptr(xyz),
                                 _lib.stream_handle(depth.device))
    _lib.check(st, "mvs_backproject_fwd")
    return xyz


@backproject_op.register_fake
def _(depth, K, R, T):
    n, _, h, w = depth.shape
    return depth.new_empty((n, h, w, 3), dtype=_F32)


def backproject(depth, K, R, T):
    """xyz fp32 [N, h, w, 3]: the world point of every pixel of depth fp32 [N, 1, h, w] (device) under the cameras
    K, R [N, 3, 3], T [N, 3, 1] (host or device); three zeros where the depth is not > 0.  Not differentiable."""
    depth = _depth_maps(depth.detach(), "backproject")
    K, R, T = _view_cams(K.detach(), R.detach(), T.detach(), depth.device, depth.shape[0], "backproject")
    return backproject_op(depth, K, R, T)


def point_cloud(depth, mask, K, R, T, colors=None):
    """points [M, 3] fp32 in world coordinates: the back-projection of the pixels of depth [N, 1, h, w] that ``mask``
    (bool [N, 1, h, w]) keeps, in view, row, column order; with colors [N, 3, h, w] also their colours [M, 3], in
    the same order.  One kernel over all pixels, then one boolean index.

    There is no cross-view de-duplication: each view contributes its own surviving pixels, so a surface point seen
    consistently by several views appears once per view; fused_point_cloud emits it once."""
    xyz = backproject(depth, K, R, T)
    if mask.shape != depth.shape or mask.dtype != torch.bool:
        raise ValueError("mask must be bool %s, got %s %s" % (tuple(depth.shape), mask.dtype, tuple(mask.shape)))
    keep = mask.to(xyz.device)[:, 0]
    points = xyz[keep]
    if colors is None:
        return points
    if colors.dim() != 4 or colors.shape[0] != depth.shape[0] or colors.shape[2:] != depth.shape[2:]:
        raise ValueError("colors must be [N, C, h, w] over the depth maps %s, got %s"
                         % (tuple(depth.shape), tuple(colors.shape)))
    return points, colors.to(xyz.device).permute(0, 2, 3, 1)[keep]


# ----------------------------------------------------------------------------------------------
# mvs_fusion::fuse_views
# ----------------------------------------------------------------------------------------------
@torch.library.custom_op("mvs_fusion::fuse_views", mutates_args=())
def fuse_views_op(depth: torch.Tensor, mask: torch.Tensor, colors: Optional[torch.Tensor], K: torch.Tensor,
                  R: torch.Tensor, T: torch.Tensor, pairs: torch.Tensor, matrices: torch.Tensor, px_thresh: float,
                  rel_thresh: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(emitted bool [N, h, w], n_merged int32 [N, h, w], xyz fp32 [N, h, w, 3], rgb fp32 [N, h, w, 3] or an empty
    tensor without colors) of depth fp32 [N, 1, h, w], mask bool or uint8 [N, 1, h, w] (non-zero keeps), colors fp32
    [N, 3, h, w] or None, the cameras, pairs int32 [N, S] and the matrices view_pair_matrices formed for them, all
    on one device.  Views go in index order, one launch each on the current stream; the workspace is allocated and
    zeroed by the call.  (mvs_fuse_views_fwd)"""
    depth = _depth_maps(depth, "fuse_views")
    lib = _lib.load()
    n, _, h, w = depth.shape
    dev = depth.device
    if tuple(mask.shape) != (n, 1, h, w) or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
        raise ValueError("mask must be bool or uint8 %s on the depth maps' device, got %s %s on %s"
                         % ((n, 1, h, w), mask.dtype, tuple(mask.shape), mask.device))
    if colors is not None and (tuple(colors.shape) != (n, 3, h, w) or colors.dtype != _F32 or colors.device != dev):
        raise ValueError("colors must be fp32 %s on the depth maps' device, got %s %s on %s"
                         % ((n, 3, h, w), colors.dtype, tuple(colors.shape), colors.device))
    if pairs.dim() != 2 or pairs.dtype != torch.int32 or pairs.device != dev or pairs.shape[0] != n:
        raise ValueError("pairs must be int32 [%d, S] on the depth maps' device, got %s %s on %s"
                         % (n, pairs.dtype, tuple(pairs.shape), pairs.device))
    s = pairs.shape[1]
    if tuple(matrices.shape) != (n, s, 24) or matrices.dtype != torch.float64 or matrices.device != dev:
        raise ValueError("matrices must be float64 [%d, %d, 24] on the depth maps' device, got %s %s on %s"
                         % (n, s, matrices.dtype, tuple(matrices.shape), matrices.device))
    for v, name in ((px_thresh, "px_thresh"), (rel_thresh, "rel_thresh")):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError("fuse_views: %s must be finite and > 0, got %r" % (name, v))
    K, R, T = _view_cams(K, R, T, dev, n, "fuse_views")
    mask, pairs, matrices = mask.contiguous(), pairs.contiguous(), matrices.contiguous()
    colors = None if colors is None else colors.contiguous()
    used = torch.empty((lib.mvs_fuse_views_workspace_bytes(n, h, w),), device=dev, dtype=torch.uint8)
    emitted = torch.empty((n, h, w), device=dev, dtype=torch.bool)
    merged = torch.empty((n, h, w), device=dev, dtype=torch.int32)
    xyz = torch.empty((n, h, w, 3), device=dev, dtype=_F32)
    rgb = torch.empty((n, h, w, 3) if colors is not None else (0,), device=dev, dtype=_F32)
    null = ctypes.c_void_p(0)
    st = lib.mvs_fuse_views_fwd(_lib.ptr(depth), _lib.ptr(mask), null if colors is None else _lib.ptr(colors),
                                _lib.ptr(K), _lib.ptr(R), _lib.ptr(T), _lib.ptr(pairs), _lib.ptr(matrices), n, s, h, w,
                                float(px_thresh), float(rel_thresh), _lib.ptr(used), _lib.ptr(emitted),
                                _lib.ptr(merged), _lib.ptr(xyz), null if colors is None else _lib.ptr(rgb),
                                _lib.stream_handle(dev))
    _lib.check(st, "mvs_fuse_views_fwd")
    return emitted, merged, xyz, rgb


@fuse_views_op.register_fake
def _(depth, mask, colors, K, R, T, pairs, matrices, px_thresh, rel_thresh):
    n, _, h, w = depth.shape
    return (depth.new_empty((n, h, w), dtype=torch.bool), depth.new_empty((n, h, w), dtype=torch.int32),
            depth.new_empty((n, h, w, 3), dtype=_F32),
            depth.new_empty((n, h, w, 3) if colors is not None else (0,), dtype=_F32))


def fused_point_cloud(depth, mask, K, R, T, pairs, colors=None, px_thresh=1.0, rel_thresh=0.01, return_counts=False):
    """points [M, 3] fp32 in world coordinates with each surface point emitted once across the views of a scan, in
    view, row, column order like point_cloud; with colors fp32 [N, 3, h, w] also their colours [M, 3] fp32, and with
    return_counts also n_merged int32 [M] (the order of the result: points, colors, n_merged).

    depth [N, 1, h, w] fp32 on the device and mask bool [N, 1, h, w] (what filter_depth returns: its depth_avg or
    the raw maps, and its mask); the cameras and ``pairs`` as geometric_consistency takes them.  Views go in index
    order (permute the inputs for another order).  A pixel of view n is emitted when the mask keeps it, its depth
    is > 0 and no earlier view has absorbed it.  It merges every source that agrees with it after
    geometric_consistency's round trip (same px_thresh / rel_thresh gates, in float64) and absorbs the source pixel
    nearest to where it lands there, which that view then does not emit.  Its point is the back-projection of
    (d + the sum of the merged d_r) / (1 + n_merged), its colour the mean of its own and the merged sources'
    bilinear colours.  A source pixel that an earlier view has absorbed may still contribute to an average: the
    result does not depend on the order in which the pixels of one view run.  One launch per view, one boolean
    index; not differentiable."""
    n = depth.shape[0] if isinstance(depth, torch.Tensor) and depth.dim() else 0
    table = pair_table(pairs, n)
    depth = _depth_maps(depth.detach(), "fused_point_cloud")
    if mask.shape != depth.shape or mask.dtype != torch.bool:
        raise ValueError("mask must be bool %s, got %s %s" % (tuple(depth.shape), mask.dtype, tuple(mask.shape)))
    if colors is not None:
        if colors.dim() != 4 or colors.shape[0] != n or colors.shape[1] != 3 or colors.shape[2:] != depth.shape[2:]:
            raise ValueError("colors must be [N, 3, h, w] over the depth maps %s, got %s"
                             % (tuple(depth.shape), tuple(colors.shape)))
        colors = colors.detach().to(device=depth.device, dtype=_F32)
    K, R, T = _view_cams(K.detach(), R.detach(), T.detach(), depth.device, n, "fused_point_cloud")
    table = table.to(depth.device)
    matrices = view_pair_matrices(K, R, T, table)
    emitted, merged, xyz, rgb = fuse_views_op(depth, mask.detach().to(depth.device), colors, K, R, T, table, matrices,
                                              float(px_thresh), float(rel_thresh))
    out = [xyz[emitted]]
    if colors is not None:
        out.append(rgb[emitted])
    if return_counts:
        out.append(merged[emitted])
    return out[0] if len(out) == 1 else tuple(out)


def write_ply(path, points, colors=None):
    """Binary little-endian PLY: ``points`` [M, 3] as float x, y, z and, when given, ``colors`` [M, 3] as uchar red,
    green, blue (an integer array is taken as 0..255, a floating one as 0..1).  Tensors or arrays; no dependency."""
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    pts = as_np(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [M, 3], got %s" % (pts.shape,))
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % pts.shape[0],
              "property float x", "property float y", "property float z"]
    if colors is not None:
        col = as_np(colors)
        if col.shape != pts.shape:
            raise ValueError("colors must be %s, got %s" % (pts.shape, col.shape))
        if col.dtype.kind == "f":
            col = np.rint(np.clip(col, 0.0, 1.0) * 255.0)
        col = np.clip(col, 0, 255).astype(np.uint8)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(pts.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = pts[:, k]
    if colors is not None:
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = col[:, k]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """(points float32 [M, 3], colors uint8 [M, 3] or None) of a PLY file, what write_ply writes and what ground-truth
    clouds come as: ``binary_little_endian`` or ``ascii``, ``vertex`` the first element, scalar vertex properties of
    any PLY type; x, y, z are read from float or double, red, green, blue when all three are there, other vertex
    properties are skipped and later elements (faces) ignored.  ValueError for a list property inside ``vertex``, a
    big-endian file and a body shorter than its header says.  Numpy only."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError("%s: not a PLY file" % path)
    body = data.find(b"\n", end) + 1
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()[1:]]
    lines = [ln for ln in lines if ln and ln[0] not in ("comment", "obj_info")]
    if not lines or lines[0][0] != "format" or len(lines[0]) < 2:
        raise ValueError("%s: no format line" % path)
    fmt = lines[0][1]
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError("%s: format %s is not supported (binary_little_endian and ascii are)" % (path, fmt))
    if len(lines) < 2 or lines[1][:2] != ["element", "vertex"] or len(lines[1]) != 3:
        raise ValueError("%s: vertex must be the first element" % path)
    count, fields = int(lines[1][2]), []
    for ln in lines[2:]:
        if ln[0] == "element":
            break
        if ln[0] != "property":
            raise ValueError("%s: unexpected header line %r" % (path, " ".join(ln)))
        if ln[1] == "list":
            raise ValueError("%s: a list property inside vertex is not supported" % path)
        if len(ln) != 3 or ln[1] not in _PLY_TYPES:
            raise ValueError("%s: unknown property %r" % (path, " ".join(ln)))
        fields.append((ln[2], "<" + _PLY_TYPES[ln[1]]))
    names = [n for n, _ in fields]
    if len(set(names)) != len(names) or not all(k in names for k in "xyz"):
        raise ValueError("%s: vertex needs properties x, y and z, each once" % path)
    if any(dict(fields)[k] not in ("<f4", "<f8") for k in "xyz"):
        raise ValueError("%s: x, y, z must be float or double" % path)
    dtype = np.dtype(fields)
    if fmt == "ascii":
        tokens = data[body:].split()
        if len(tokens) < count * len(fields):
            raise ValueError("%s: the body ends before %d vertices" % (path, count))
        table = np.array(tokens[:count * len(fields)], dtype="S").reshape(count, len(fields))
        rec = np.empty(count, dtype=dtype)
        for k, (name, kind) in enumerate(fields):
            rec[name] = table[:, k].astype(np.float64).astype(kind)
    else:
        if len(data) - body < count * dtype.itemsize:
            raise ValueError("%s: the body ends before %d vertices" % (path, count))
        rec = np.frombuffer(data, dtype=dtype, count=count, offset=body)
    points = np.stack([rec[k].astype(np.float32) for k in "xyz"], 1).reshape(count, 3)
    if not all(k in names for k in ("red", "green", "blue")):
        return points, None
    return points, np.stack([rec[k].astype(np.uint8) for k in ("red", "green", "blue")], 1).reshape(count, 3)
