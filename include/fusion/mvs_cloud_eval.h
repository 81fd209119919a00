/* mvs_cloud_eval.h -- nearest-neighbour distances between two point clouds in libmvs_cost_volume.so: what the
 * accuracy / completeness and precision / recall of a reconstructed cloud are built from (mvs_amd/cloud_eval.py;
 * kernels: csrc/cloud_nn.hip).
 *
 * The conventions of mvs_depth_filter.h hold: additive (mvs_abi_version() is unchanged), every pointer a DEVICE
 * pointer, `stream` a hipStream_t (NULL: the default stream), nothing allocates or synchronises, no atomics, every
 * output element is written once.
 *
 * THE DEFINITION (it does not depend on the grid).  query [m][3] and target [g][3] fp32, max_dist finite and > 0; all
 * arithmetic in float64 on the widened fp32 coordinates.
 *   d2(i, j)  = dx dx + dy dy + dz dz, one expression for every path (the kernel fuses the products in this order)
 *   candidate   a target j with three finite coordinates and d2(i, j) <= max_dist^2 (written !(a <= b) -> skip, so a
 *               NaN fails it)
 *   best(i)   = the minimum of d2(i, j) over the candidates
 *   index[i]  = the lowest j among the candidates with d2(i, j) == best(i), in the caller's order of the targets
 *   dist[i]   = sqrt(best(i)), rounded once to fp32
 *   no candidate, or a query with a non-finite coordinate: dist = +inf, index = -1
 *
 * THE GRID.  nx ny nz cells of edge `cell` from `origin`; a point's cell coordinate per axis is
 * floor((p - origin) / cell) in float64, clamped to the grid on the double before the integer conversion; its key is
 * (cz ny + cy) nx + cx, or ncells = nx ny nz for a non-finite point.  The grid must cover the finite targets
 * ((p - origin) / cell within [0, n] per axis: the clamp is for the rounding at the faces only); queries may lie
 * anywhere.  Steps of a search:
 *   1. mvs_cloud_cell_keys on the targets; sort the keys (stable) and gather the targets and their indices into that
 *      order; mvs_cloud_cell_ranges on the sorted keys
 *   2. mvs_cloud_cell_keys on the queries and a sort of those keys give query_order (any permutation is correct; cell
 *      order is what makes neighbouring lanes share cells)
 *   3. mvs_cloud_nearest
 *
 * Arguments are checked before any launch:
 *   MVS_ERR_INVALID_ARGUMENT  a null or misaligned pointer (4 bytes), a negative count, cell or max_dist not finite
 *                             and > 0, a grid dimension < 1, more than MVS_CLOUD_MAX_CELLS cells, more than
 *                             MVS_CLOUD_MAX_RINGS rings (ceil(max_dist / cell)), an origin that is not finite
 *   MVS_ERR_TOO_LARGE         a count or nx ny nz at or past 2^31
 */
#ifndef MVS_CLOUD_EVAL_H
#define MVS_CLOUD_EVAL_H

#include <stddef.h>

#include "mvs_depth_filter.h"

#define MVS_CLOUD_MAX_CELLS (1 << 27)
#define MVS_CLOUD_MAX_RINGS 64

#ifdef __cplusplus
extern "C" {
#endif

/* The bytes of the cell table, (nx ny nz + 1) int32 (host only); 0 for a grid the calls would refuse. */
size_t mvs_cloud_cell_table_bytes(int nx, int ny, int nz);

/* points [n][3] fp32 -> keys [n] int32, one thread per point.  n == 0 launches nothing. */
int mvs_cloud_cell_keys(const float* points, long long n, double origin_x, double origin_y, double origin_z,
                        double cell, int nx, int ny, int nz, int* keys, void* stream);

/* sorted_keys [n] ascending in [0, ncells] -> cell_start [ncells + 1] int32: cell k holds the sorted positions
 * cell_start[k] .. cell_start[k + 1] - 1, and cell_start[ncells] is the number of finite points.  One thread per
 * position i writes i to every k in (key[i - 1], key[i]] (the first from k = 0), the last also n to every k in
 * (key[n - 1], ncells]: every entry once, no memset (n == 0 has no position to write from: the table is zeroed). */
int mvs_cloud_cell_ranges(const int* sorted_keys, long long n, long long ncells, int* cell_start, void* stream);

/* query [m][3] and query_order [m] (a permutation of 0 .. m - 1); targets [g][3] in cell order, target_index [g]
 * their indices in the caller's order, cell_start as written by mvs_cloud_cell_ranges for the same grid.  Per query:
 * the rings of Chebyshev radius r = 0 .. ceil(max_dist / cell) around its (unclamped) cell, intersected with the
 * grid; it stops after ring r once best <= (r cell (1 - 2^-23))^2, which only ever looks further than r cell.
 * dist [m] fp32 and index [m] int32 in the caller's order of the queries.  m == 0 launches nothing; g == 0 fills
 * dist / index with +inf / -1 without a search. */
int mvs_cloud_nearest(const float* query, const int* query_order, long long m, const float* targets,
                      const int* target_index, long long g, const int* cell_start, double origin_x, double origin_y,
                      double origin_z, double cell, int nx, int ny, int nz, double max_dist, float* dist, int* index,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_CLOUD_EVAL_H */
