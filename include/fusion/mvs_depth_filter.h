/* mvs_depth_filter.h -- depth-map filtering and fusion in libmvs_cost_volume.so: what an MVSNet pipeline does with the
 * depth maps of a scan's N views (mvs_amd/fusion.py; kernels: csrc/depth_filter.hip).
 *
 * Additive: mvs_abi_version() is unchanged.  Status codes, pointer and stream conventions are those of
 * mvs_cost_volume.h: every pointer is a DEVICE pointer, 4-byte aligned (8-byte for doubles), `stream` is a
 * hipStream_t (NULL: the default stream), nothing allocates or synchronises, every output element is written once
 * with a plain store (no atomics, nothing to zero).  Arguments are checked before any launch:
 *   MVS_ERR_INVALID_ARGUMENT  a null or misaligned pointer, a dimension <= 0, d_num < 2, n_slots > 64, a threshold
 *                             that is not finite and > 0
 *   MVS_ERR_TOO_LARGE         batch * h * w, n_views * h * w or n_views * n_slots at or past 2^31
 *
 * Cameras: K, R [n][3][3], T [n][3] fp32 with x_cam = R x_world + T, K for the map's own resolution, pixel (x, y) =
 * integer column and row indices.  A depth is valid when it is > 0 (0, negative and NaN are not).
 *
 * The last stage, the cloud with each surface point emitted once across the views, is mvs_view_fusion.h.
 */
#ifndef MVS_DEPTH_FILTER_H
#define MVS_DEPTH_FILTER_H

#include <stddef.h>

#include "../mvs_cost_volume.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_FILTER_MAX_SLOTS 64
#define MVS_FILTER_PAIR_DOUBLES 24

/* Photometric confidence: MVSNet's four-plane probability sum around the estimated depth.
 * prob [batch][1][d_num][h][w], depth [batch][1][h][w], d_batch [batch][d_num] (the planes mvs_extract_depth_map_fwd
 * receives), conf [batch][1][h][w], all fp32.  Per pixel, in separately rounded fp32 operations,
 *   t = (depth - d_batch[b][0]) / (d_batch[b][1] - d_batch[b][0]),   k0 = floor(t) clamped to [0, d_num - 1],
 *   conf = sum of prob[k] over k = k0 - 1 .. k0 + 2 with 0 <= k < d_num, added in ascending k.
 * A NaN t (a NaN depth; planes 0 and 1 coinciding at the depth) gives conf = 0. */
int mvs_photometric_confidence_fwd(const float* prob, const float* depth, const float* d_batch, int batch, int d_num,
                                   int h, int w, float* conf, void* stream);

/* The matrices of every (view, source slot) pair, in fp64: pairs [n_views][n_slots] int32 names each view's sources;
 * -1 (any value outside [0, n_views)) or the view itself is an empty slot.  matrices [n_views][n_slots][24] doubles:
 *   [0..8]  M  = K_s R_s R_n^T K_n^-1      [9..11]  m  = K_s (T_s - R_s R_n^T T_n)      view n -> source s
 *   [12..20] M' = K_n R_n R_s^T K_s^-1     [21..23] m' = K_n (T_n - R_n R_s^T T_s)      and back
 * (zeros for an empty slot).  mvs_view_pair_matrices_bytes (host only) = n_views * n_slots * 24 * 8, 0 for
 * dimensions the call would refuse. */
size_t mvs_view_pair_matrices_bytes(int n_views, int n_slots);
int mvs_view_pair_matrices(const float* K, const float* R, const float* T, const int* pairs, int n_views,
                           int n_slots, double* matrices, void* stream);

/* Geometric consistency of depth [n_views][1][h][w] (each view's map in its own camera).  Per pixel (x, y) of view n
 * with valid depth d and per non-empty slot, all in fp64:
 *   1. p = d M (x, y, 1)^T + m; p.z > 0; xs = p.x / p.z, ys = p.y / p.z
 *   2. x0 = floor(xs), y0 = floor(ys); the taps (x0 .. x0 + 1, y0 .. y0 + 1) of the source's map all inside it and
 *      valid; d_s = (1 - fy) ((1 - fx) t00 + fx t01) + fy ((1 - fx) t10 + fx t11), fx = xs - x0, fy = ys - y0
 *   3. q = d_s M' (xs, ys, 1)^T + m'; q.z > 0; xr = q.x / q.z, yr = q.y / q.z, d_r = q.z
 *   4. consistent iff (xr - x)^2 + (yr - y)^2 < px_thresh^2 and |d_r - d| < rel_thresh d
 * (a NaN fails every comparison).  n_consistent [n_views][1][h][w] int32 = the number of consistent slots;
 * depth_avg fp32 = (d + sum of the consistent d_r, in slot order) / (1 + n_consistent), fp64 rounded once.  An
 * invalid pixel gets 0 in both.  `pairs` and `matrices` as given to / written by mvs_view_pair_matrices. */
int mvs_geometric_consistency_fwd(const float* depth, const int* pairs, const double* matrices, int n_views,
                                  int n_slots, int h, int w, double px_thresh, double rel_thresh, int* n_consistent,
                                  float* depth_avg, void* stream);

/* Back-projection: xyz [n_views][h][w][3] fp32 = R_n^T (d K_n^-1 (x, y, 1)^T - T_n), fp64 rounded once; three zeros
 * for an invalid d. */
int mvs_backproject_fwd(const float* depth, const float* K, const float* R, const float* T, int n_views, int h,
                        int w, float* xyz, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_DEPTH_FILTER_H */
