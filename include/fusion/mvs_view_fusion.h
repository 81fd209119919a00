/* mvs_view_fusion.h -- the fused point cloud of a scan in libmvs_cost_volume.so: each surface point emitted once
 * across the N views (mvs_amd/fusion.py fused_point_cloud; kernel: csrc/depth_fuse.hip).
 *
 * The last stage on top of mvs_depth_filter.h, whose conventions hold here: additive (mvs_abi_version() is
 * unchanged), every pointer a DEVICE pointer, `stream` a hipStream_t (NULL: the default stream), nothing allocates
 * or synchronises, no atomics.  Arguments are checked before any launch:
 *   MVS_ERR_INVALID_ARGUMENT  a null or misaligned pointer (byte buffers: any address; floats and ints 4 bytes; the
 *                             matrices 8), colors and rgb not both null or both non-null, a dimension <= 0,
 *                             n_slots > 64, a threshold that is not finite and > 0
 *   MVS_ERR_TOO_LARGE         n_views * h * w or n_views * n_slots at or past 2^31
 * (A header of its own: mvs_depth_filter.h keeps its five declarations, name for name.)
 */
#ifndef MVS_VIEW_FUSION_H
#define MVS_VIEW_FUSION_H

#include <stddef.h>

#include "mvs_depth_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The bytes of the `used` workspace, n_views * h * w (host only); 0 for dimensions the call would refuse. */
size_t mvs_fuse_views_workspace_bytes(int n_views, int h, int w);

/* depth [n_views][1][h][w] fp32; mask [n_views][1][h][w], one byte per pixel, non-zero = keep; colors
 * [n_views][3][h][w] fp32 or NULL; K, R, T as in mvs_depth_filter.h; pairs [n_views][n_slots] and matrices as given
 * to / written by mvs_view_pair_matrices.  used [n_views][h][w] bytes: workspace, zeroed by the call on `stream`
 * before the first view.  Views go in index order n = 0 .. n_views - 1, one launch per view on `stream`, one thread
 * per pixel (x, y) of view n:
 *   1. emitted = mask != 0 and depth > 0 and used[n][y][x] == 0.  A pixel that is not emitted gets 0 in emitted,
 *      n_merged, xyz and rgb.
 *   2. per non-empty slot, steps 1-4 of mvs_geometric_consistency_fwd (fp64, the same comparisons, taps and round
 *      trip); a slot that passes is merged.
 *   3. per merged slot with source view s and position (xs, ys): used[s][floor(ys + 0.5)][floor(xs + 0.5)] = 1, a
 *      plain byte store (the indices, inside the map by step 2's tap test, are clamped on the doubles first).
 *   4. n_merged = the number of merged slots; d_m = (d + sum of the merged d_r, in slot order) / (1 + n_merged),
 *      fp64, not rounded.
 *   5. xyz = R_n^T (d_m K_n^-1 (x, y, 1)^T - T_n), fp64 rounded once.
 *   6. with colors, per channel: rgb = (c_n(x, y) + sum over the merged slots of c_s blended at (xs, ys) with the
 *      four taps and weights of d_s) / (1 + n_merged), fp64 in slot order, rounded once.
 * A launch reads `used` only for its own view and writes it only for other views; the source's `used` flags are
 * not read when merging (an absorbed source pixel still contributes to an average), so the result does not vary
 * from run to run.  emitted [n_views][h][w] bytes (0 / 1), n_merged [n_views][h][w] int32, xyz and rgb
 * [n_views][h][w][3] fp32 (rgb NULL exactly when colors is); every output element is written once. */
int mvs_fuse_views_fwd(const float* depth, const unsigned char* mask, const float* colors, const float* K,
                       const float* R, const float* T, const int* pairs, const double* matrices, int n_views,
                       int n_slots, int h, int w, double px_thresh, double rel_thresh, unsigned char* used,
                       unsigned char* emitted, int* n_merged, float* xyz, float* rgb, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_VIEW_FUSION_H */
