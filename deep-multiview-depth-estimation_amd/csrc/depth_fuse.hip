// depth_fuse.hip -- the last stage of depth-map fusion: every surface point of a scan emitted once across its N views
// (include/fusion/mvs_view_fusion.h; mvs_amd/fusion.py fused_point_cloud).
//
// Views go in index order, one launch per view on the caller's stream.  A pixel of view n is emitted when its mask
// keeps it and no earlier view has absorbed it (used[n] == 0); it absorbs, in every source view that agrees with it
// after the round trip of depth_filter.hip's consistency kernel, the pixel nearest to where it lands (used[s] = 1),
// and its point and colour are the averages over itself and the agreeing sources.  A launch reads `used` only for
// its own view and writes it only for other views (a slot naming the view itself is empty), several threads may
// store the same 1 to one byte, and the order between launches is the stream's: deterministic without atomics.
//
// One thread per pixel, 64-thread workgroups, size_t offsets, the geometry in fp64, every output element written
// once with a plain vector store, as depth_filter.hip.  The per-slot round trip restates that file's steps 1-4 (a
// translation unit of its own: the code objects of the sibling kernels do not change).
#include "launchers.h"
#include "sampling_matrix.h"

namespace mvs {
namespace {

constexpr int kFuseBlock = 64;

// a slot's source view, or -1: the slot is empty (-1), names the view itself, or names no view at all
__device__ inline int fuse_slot_source(const int* __restrict__ pairs, int N, int S, int n, int s) {
  const int v = pairs[(size_t)n * S + s];
  return (v < 0 || v >= N || v == n) ? -1 : v;
}

// the four-tap blend of depth_filter.hip step 2, on a map whose taps are known to be inside it
__device__ inline double blend4(const float* __restrict__ sp, int w, double fx, double fy) {
  return (1.0 - fy) * ((1.0 - fx) * (double)sp[0] + fx * (double)sp[1]) +
         fy * ((1.0 - fx) * (double)sp[w] + fx * (double)sp[w + 1]);
}

// View n of depth [N][1][h][w], mask [N][1][h][w] bytes, colors [N][3][h][w] or null; used [N][h][w] bytes; outputs
// emitted [N][h][w] bytes, merged [N][h][w] int32, xyz [N][h][w][3], rgb [N][h][w][3] or null.
__global__ __launch_bounds__(kFuseBlock) void fuse_view_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ mask, const float* __restrict__ colors,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ T,
    const int* __restrict__ pairs, const double* __restrict__ mats, int N, int S, int h, int w, int n, double px2,
    double rel, uint8_t* used, uint8_t* __restrict__ emitted, int* __restrict__ merged, float* __restrict__ xyz,
    float* __restrict__ rgb) {
  const uint32_t hw = (uint32_t)h * (uint32_t)w;
  const uint32_t p = blockIdx.x * (uint32_t)kFuseBlock + threadIdx.x;
  if (p >= hw) return;
  const size_t e = (size_t)n * hw + p;
  const int yi = (int)(p / (uint32_t)w), xi = (int)(p - (uint32_t)yi * (uint32_t)w);
  const float df = depth[e];
  float* o = xyz + e * 3;
  float* oc = rgb ? rgb + e * 3 : nullptr;
  if (!(mask[e] != 0 && df > 0.0f && used[e] == 0)) {
    emitted[e] = 0;
    merged[e] = 0;
    o[0] = 0.0f;
    o[1] = 0.0f;
    o[2] = 0.0f;
    if (oc) {
      oc[0] = 0.0f;
      oc[1] = 0.0f;
      oc[2] = 0.0f;
    }
    return;
  }
  const double d = (double)df, x = (double)xi, y = (double)yi;
  double sum = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (colors) {
    const float* cn = colors + (size_t)n * 3 * hw + p;
    c0 = (double)cn[0];
    c1 = (double)cn[hw];
    c2 = (double)cn[2 * (size_t)hw];
  }
  int cnt = 0;
  for (int s = 0; s < S; ++s) {
    const int src = fuse_slot_source(pairs, N, S, n, s);
    if (src < 0) continue;
    const double* M = mats + ((size_t)n * S + s) * 24;
    // 1. into the source view
    const double pz = d * (M[6] * x + M[7] * y + M[8]) + M[11];
    if (!(pz > 0.0)) continue;
    const double xs = (d * (M[0] * x + M[1] * y + M[2]) + M[9]) / pz;
    const double ys = (d * (M[3] * x + M[4] * y + M[5]) + M[10]) / pz;
    // 2. its depth there: four taps, all inside and valid
    const double x0 = floor(xs), y0 = floor(ys);
    if (!(x0 >= 0.0 && x0 <= (double)(w - 2) && y0 >= 0.0 && y0 <= (double)(h - 2))) continue;
    const size_t tap = (size_t)((int)y0 * w + (int)x0);
    const float* sp = depth + (size_t)src * hw + tap;
    if (!(sp[0] > 0.0f && sp[1] > 0.0f && sp[w] > 0.0f && sp[w + 1] > 0.0f)) continue;
    const double fx = xs - x0, fy = ys - y0;
    const double ds = blend4(sp, w, fx, fy);
    // 3. back into this view
    const double* Q = M + 12;
    const double qz = ds * (Q[6] * xs + Q[7] * ys + Q[8]) + Q[11];
    if (!(qz > 0.0)) continue;
    const double xr = (ds * (Q[0] * xs + Q[1] * ys + Q[2]) + Q[9]) / qz;
    const double yr = (ds * (Q[3] * xs + Q[4] * ys + Q[5]) + Q[10]) / qz;
    // 4. the two gates
    const double ex = xr - x, ey = yr - y;
    if (!(ex * ex + ey * ey < px2)) continue;
    if (!(fabs(qz - d) < rel * d)) continue;
    // merged: absorb the source pixel nearest to (xs, ys).  It is one of the four taps, so inside the map; clamped
    // on the doubles all the same before the conversion.  A view before this one has been emitted already: a mark
    // there would never be read.
    if (src > n) {
      const double xn = fmin(fmax(floor(xs + 0.5), 0.0), (double)(w - 1));
      const double yn = fmin(fmax(floor(ys + 0.5), 0.0), (double)(h - 1));
      used[(size_t)src * hw + (size_t)((int)yn * w + (int)xn)] = 1;
    }
    sum += qz;
    ++cnt;
    if (colors) {
      const float* cs = colors + (size_t)src * 3 * hw + tap;
      c0 += blend4(cs, w, fx, fy);
      c1 += blend4(cs + hw, w, fx, fy);
      c2 += blend4(cs + 2 * (size_t)hw, w, fx, fy);
    }
  }
  const double inv_cnt = (double)(1 + cnt);
  const double dm = (d + sum) / inv_cnt;
  emitted[e] = 1;
  merged[e] = cnt;
  // R_n^T (d_m K_n^-1 (x, y, 1)^T - T_n), as depth_filter.hip's back-projection
  const Mat3 Ki = mat_inv(load_mat(K + 9 * (size_t)n));
  const double rx = Ki.a[0] * x + Ki.a[1] * y + Ki.a[2], ry = Ki.a[3] * x + Ki.a[4] * y + Ki.a[5],
               rz = Ki.a[6] * x + Ki.a[7] * y + Ki.a[8];
  const float* Tn = T + 3 * (size_t)n;
  const Mat3 Rn = load_mat(R + 9 * (size_t)n);
  const double cx = dm * rx - (double)Tn[0], cy = dm * ry - (double)Tn[1], cz = dm * rz - (double)Tn[2];
  o[0] = (float)(Rn.a[0] * cx + Rn.a[3] * cy + Rn.a[6] * cz);
  o[1] = (float)(Rn.a[1] * cx + Rn.a[4] * cy + Rn.a[7] * cz);
  o[2] = (float)(Rn.a[2] * cx + Rn.a[5] * cy + Rn.a[8] * cz);
  if (oc) {
    oc[0] = (float)(c0 / inv_cnt);
    oc[1] = (float)(c1 / inv_cnt);
    oc[2] = (float)(c2 / inv_cnt);
  }
}

}  // namespace

void launch_fuse_views(const float* depth, const uint8_t* mask, const float* colors, const float* K, const float* R,
                       const float* T, const int* pairs, const double* mats, int N, int S, int h, int w,
                       double px_thresh, double rel_thresh, uint8_t* used, uint8_t* emitted, int* merged, float* xyz,
                       float* rgb, hipStream_t s) {
  const size_t hw = (size_t)h * (size_t)w;
  if (hipMemsetAsync(used, 0, (size_t)N * hw, s) != hipSuccess) return;   // (the caller's LaunchCheck reports it)
  const dim3 grid((unsigned)((hw + kFuseBlock - 1) / kFuseBlock));
  for (int n = 0; n < N; ++n)
    hipLaunchKernelGGL(fuse_view_kernel, grid, dim3(kFuseBlock), 0, s, depth, mask, colors, K, R, T, pairs, mats, N,
                       S, h, w, n, px_thresh * px_thresh, rel_thresh, used, emitted, merged, xyz, rgb);
}

}  // namespace mvs
