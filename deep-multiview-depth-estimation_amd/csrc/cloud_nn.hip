// cloud_nn.hip -- nearest-neighbour distances between two point clouds on a uniform grid: what accuracy /
// completeness (DTU) and precision / recall (Tanks and Temples) are built from (include/fusion/mvs_cloud_eval.h;
// mvs_amd/cloud_eval.py).
//
// Three kernels.  cell_keys: one thread per point, its linear cell index (ncells for a non-finite point).  cell_ranges:
// one thread per position of the sorted keys, the dense cell_start table, every entry written once.  nearest: one
// query per lane in 64-thread workgroups over the queries in cell order.  The lanes of a workgroup are served in
// groups that share a (y, z) cell row and lie within kCloudSpan cells in x; a group walks the rings of Chebyshev
// radius r = 0 .. R around its x-run of cells together.  Cells that are neighbours in x are neighbours in the sorted
// order, so a ring is a list of contiguous point ranges: each is staged through LDS in passes of kCloudPass points
// and every lane of the group reads the staged points from LDS.
//
// All pair arithmetic is fp64 on the widened fp32 coordinates, by pair_d2 alone.  The result does not depend on the
// grid: a lane stops after ring r only once no point outside the rings walked can be as near as its best (the slack
// of ring_stop), and a tie goes to the lowest original index wherever the two points lie.  size_t offsets, no
// atomics, every output element written once with a plain vector store.
#include "launchers.h"

namespace mvs {
namespace {

constexpr int kCloudBlock = 64;    // one wavefront: the group votes below are wave votes
constexpr int kCloudPass = 256;    // points per LDS staging pass (16 bytes each)
constexpr int kCloudSpan = 4;      // widest x-run of query cells served together
constexpr int kCloudLinear = 256;  // threads per workgroup of the two per-point kernels
static_assert(kCloudBlock == 64, "the nearest kernel's votes and shuffles span one 64-lane wavefront");

struct CloudGrid {
  double ox, oy, oz, cell;
  int nx, ny, nz;
};

struct alignas(16) StagedPoint {
  float x, y, z;
  int index;   // the point's index in the caller's order
};

__device__ inline bool finite3(float x, float y, float z) {
  return (x - x == 0.0f) && (y - y == 0.0f) && (z - z == 0.0f);
}

// floor((p - origin) / cell) in fp64, clamped to [lo, hi] on the double before the conversion
__device__ inline int cell_coord(float p, double origin, double cell, double lo, double hi) {
  return (int)fmin(fmax(floor(((double)p - origin) / cell), lo), hi);
}

// THE pair distance: dx dx + dy dy + dz dz with the products fused in this order, for every path
__device__ inline double pair_d2(double qx, double qy, double qz, float tx, float ty, float tz) {
  const double dx = qx - (double)tx, dy = qy - (double)ty, dz = qz - (double)tz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

// A lane may stop after ring r when best <= ring_stop(r): a point in no ring <= r differs from the query's cell by
// more than r on some axis, so it is farther than r cell less the rounding of the two cell assignments, at most
// 2^-51 (n + R + 2) <= 2^-23 of a cell on that axis.  r = 0 gives 0: only an exact hit stops.
__device__ inline double ring_stop(int r, double cell) {
  const double reach = (double)r * cell * (1.0 - 0x1p-23);
  return reach * reach;
}

__global__ __launch_bounds__(kCloudLinear) void cloud_cell_keys_kernel(const float* __restrict__ points, int n,
                                                                       CloudGrid g, int* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * kCloudLinear + threadIdx.x;
  if (i >= (size_t)n) return;
  const float* p = points + i * 3;
  const float x = p[0], y = p[1], z = p[2];
  int key = g.nx * g.ny * g.nz;
  if (finite3(x, y, z)) {
    const int cx = cell_coord(x, g.ox, g.cell, 0.0, (double)(g.nx - 1));
    const int cy = cell_coord(y, g.oy, g.cell, 0.0, (double)(g.ny - 1));
    const int cz = cell_coord(z, g.oz, g.cell, 0.0, (double)(g.nz - 1));
    key = (cz * g.ny + cy) * g.nx + cx;
  }
  keys[i] = key;
}

// sorted keys in [0, ncells] -> cell_start [ncells + 1]: position i writes i to every k in (key[i - 1], key[i]] (the
// first from 0), the last position also n to every k in (key[n - 1], ncells]
__global__ __launch_bounds__(kCloudLinear) void cloud_cell_ranges_kernel(const int* __restrict__ keys, int n,
                                                                         int ncells, int* __restrict__ cell_start) {
  const size_t i = (size_t)blockIdx.x * kCloudLinear + threadIdx.x;
  if (i >= (size_t)n) return;
  const int hi = min(max(keys[i], 0), ncells);
  const int lo = i ? min(max(keys[i - 1], 0), ncells) + 1 : 0;
  for (int k = lo; k <= hi; ++k) cell_start[k] = (int)i;
  if (i + 1 == (size_t)n)
    for (int k = hi + 1; k <= ncells; ++k) cell_start[k] = n;
}

__global__ __launch_bounds__(kCloudLinear) void cloud_no_target_kernel(int m, float* __restrict__ dist,
                                                                       int* __restrict__ index) {
  const size_t i = (size_t)blockIdx.x * kCloudLinear + threadIdx.x;
  if (i >= (size_t)m) return;
  dist[i] = INFINITY;
  index[i] = -1;
}

__device__ inline int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// query [m][3] in the caller's order, query_order [m] the queries in cell order; targets [g][3] in cell order with
// target_index [g] their indices in the caller's order; cell_start [ncells + 1]
__global__ __launch_bounds__(kCloudBlock) void cloud_nearest_kernel(
    const float* __restrict__ query, const int* __restrict__ query_order, int m, const float* __restrict__ targets,
    const int* __restrict__ target_index, int n_targets, const int* __restrict__ cell_start, CloudGrid g, int rings,
    double max2, float* __restrict__ dist, int* __restrict__ index) {
  __shared__ StagedPoint staged[kCloudPass];
  const int lane = threadIdx.x;
  const size_t slot = (size_t)blockIdx.x * kCloudBlock + lane;
  int qi = -1, cx = 0, cy = 0, cz = 0;
  double qx = 0.0, qy = 0.0, qz = 0.0;
  bool pending = false;
  if (slot < (size_t)m) {
    qi = min(max(query_order[slot], 0), m - 1);
    const float* q = query + (size_t)qi * 3;
    const float x = q[0], y = q[1], z = q[2];
    if (finite3(x, y, z)) {
      pending = true;
      qx = (double)x, qy = (double)y, qz = (double)z;
      // the unclamped cell; past R + 1 cells outside the grid nothing is within max_dist, so the bound is harmless
      const double out = (double)(rings + 2);
      cx = cell_coord(x, g.ox, g.cell, -out, (double)g.nx + out);
      cy = cell_coord(y, g.oy, g.cell, -out, (double)g.ny + out);
      cz = cell_coord(z, g.oz, g.cell, -out, (double)g.nz + out);
    }
  }
  double best = INFINITY;
  int best_index = -1;
  for (;;) {
    const unsigned long long waiting = __ballot(pending);
    if (!waiting) break;
    // the group: the first waiting lane's (y, z) row, kCloudSpan cells in x from its cell
    const int lead = __ffsll(waiting) - 1;
    const int gx = __builtin_amdgcn_readfirstlane(__shfl(cx, lead, 64));
    const int gy = __builtin_amdgcn_readfirstlane(__shfl(cy, lead, 64));
    const int gz = __builtin_amdgcn_readfirstlane(__shfl(cz, lead, 64));
    const bool mine = pending && cy == gy && cz == gz && cx >= gx && cx < gx + kCloudSpan;
    const int gx1 = __builtin_amdgcn_readfirstlane(wave_max(mine ? cx : gx));
    bool done = !mine;
    for (int r = 0; r <= rings && !__all(done); ++r) {
      const int z0 = max(gz - r, 0), z1 = min(gz + r, g.nz - 1);
      const int y0 = max(gy - r, 0), y1 = min(gy + r, g.ny - 1);
      for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y) {
          // a row on the ring's shell brings its whole x-run, a row inside it the two end cells
          const bool shell = r == 0 || abs(z - gz) == r || abs(y - gy) == r;
          const size_t row = ((size_t)z * g.ny + y) * g.nx;
          for (int part = 0; part < (shell ? 1 : 2); ++part) {
            const int xa = max(shell || part == 0 ? gx - r : gx1 + r, 0);
            const int xb = min(shell || part == 1 ? gx1 + r : gx - r, g.nx - 1);
            if (xa > xb) continue;
            const int begin = max(cell_start[row + xa], 0), end = min(cell_start[row + xb + 1], n_targets);
            for (int base = begin; base < end; base += kCloudPass) {
              const int count = min(kCloudPass, end - base);
              __syncthreads();
              for (int k = lane; k < count; k += kCloudBlock) {
                const size_t j = (size_t)base + k;
                const float* t = targets + j * 3;
                staged[k] = StagedPoint{t[0], t[1], t[2], target_index[j]};
              }
              __syncthreads();
              if (done) continue;
              for (int k = 0; k < count; ++k) {
                const StagedPoint t = staged[k];
                const double d2 = pair_d2(qx, qy, qz, t.x, t.y, t.z);
                if (!(d2 <= max2)) continue;
                if (d2 < best || (d2 == best && t.index < best_index)) {
                  best = d2;
                  best_index = t.index;
                }
              }
            }
          }
        }
      if (!done) done = best <= ring_stop(r, g.cell);
    }
    if (mine) pending = false;
  }
  if (qi >= 0) {
    dist[qi] = best_index >= 0 ? (float)sqrt(best) : INFINITY;
    index[qi] = best_index;
  }
}

inline dim3 linear_grid(int n) { return dim3((unsigned)(((size_t)n + kCloudLinear - 1) / kCloudLinear)); }

}  // namespace

void launch_cloud_cell_keys(const float* points, int n, double ox, double oy, double oz, double cell, int nx, int ny,
                            int nz, int* keys, hipStream_t s) {
  hipLaunchKernelGGL(cloud_cell_keys_kernel, linear_grid(n), dim3(kCloudLinear), 0, s, points, n,
                     CloudGrid{ox, oy, oz, cell, nx, ny, nz}, keys);
}

void launch_cloud_cell_ranges(const int* sorted_keys, int n, int ncells, int* cell_start, hipStream_t s) {
  if (n == 0) {   // no position to write from: the table of an empty cloud is all zeros
    (void)hipMemsetAsync(cell_start, 0, ((size_t)ncells + 1) * sizeof(int), s);   // (the caller's LaunchCheck reports)
    return;
  }
  hipLaunchKernelGGL(cloud_cell_ranges_kernel, linear_grid(n), dim3(kCloudLinear), 0, s, sorted_keys, n, ncells,
                     cell_start);
}

void launch_cloud_nearest(const float* query, const int* query_order, int m, const float* targets,
                          const int* target_index, int n_targets, const int* cell_start, double ox, double oy,
                          double oz, double cell, int nx, int ny, int nz, int rings, double max_dist, float* dist,
                          int* index, hipStream_t s) {
  if (n_targets == 0) {
    hipLaunchKernelGGL(cloud_no_target_kernel, linear_grid(m), dim3(kCloudLinear), 0, s, m, dist, index);
    return;
  }
  const dim3 grid((unsigned)(((size_t)m + kCloudBlock - 1) / kCloudBlock));
  hipLaunchKernelGGL(cloud_nearest_kernel, grid, dim3(kCloudBlock), 0, s, query, query_order, m, targets,
                     target_index, n_targets, cell_start, CloudGrid{ox, oy, oz, cell, nx, ny, nz}, rings,
                     max_dist * max_dist, dist, index);
}

}  // namespace mvs
