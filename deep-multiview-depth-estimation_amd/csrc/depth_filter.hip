// depth_filter.hip -- what follows the network in an MVSNet pipeline: the photometric confidence of a depth map, the
// cross-view geometric consistency of the N depth maps of a scan, and the back-projection of the pixels that survive
// (include/fusion/mvs_depth_filter.h; mvs_amd/fusion.py).  The reference stops at the depth maps.
//
// One thread per output pixel, 64-thread workgroups (soft_argmin.hip: the pixels of a small map spread over every
// CU), every output element written once with a plain vector store: no atomics, nothing zeroed, no host
// synchronisation.  The geometry runs in fp64 per pixel: its decisions are thresholds on differences of quantities
// near 425-935 with a 1 % gate and a 1-pixel gate, which fp32 rounding would flip; a few hundred flops per pixel and
// slot on maps of 20 k-120 k pixels.  The taps of a source map are gathers from at most a few hundred KB: L2 hits.
#include "launchers.h"
#include "sampling_matrix.h"

namespace mvs {
namespace {

constexpr int kFilterBlock = 64;

inline dim3 filter_grid(size_t n) { return dim3((unsigned)((n + kFilterBlock - 1) / kFilterBlock)); }

// a. prob [B][1][D][h][w], depth [B][1][h][w], d_batch [B][D].  t = (depth - d_0) / (d_1 - d_0) in separately
// rounded fp32 operations, k0 = floor(t) clamped to [0, D - 1], conf = P[k0 - 1] + P[k0] + P[k0 + 1] + P[k0 + 2] over
// the planes that exist, added in ascending k.  A NaN t (a NaN depth, or coincident planes 0 and 1) gives 0.
__global__ __launch_bounds__(kFilterBlock) void photometric_confidence_kernel(const float* __restrict__ prob,
                                                                              const float* __restrict__ depth,
                                                                              const float* __restrict__ d_batch,
                                                                              int B, int D, uint32_t hw,
                                                                              float* __restrict__ conf) {
#pragma clang fp contract(off)   // separately rounded ops: no a * b + c fused into an fma
  const size_t e = (size_t)blockIdx.x * kFilterBlock + threadIdx.x;
  if (e >= (size_t)B * hw) return;
  const size_t b = e / hw, p = e - b * hw;
  const float* db = d_batch + b * D;
  const float d0 = db[0];
  const float t = (depth[e] - d0) / (db[1] - d0);
  if (!(t == t)) {
    conf[e] = 0.0f;
    return;
  }
  const float tf = floorf(t);
  const int k0 = !(tf > 0.0f) ? 0 : (tf >= (float)(D - 1) ? D - 1 : (int)tf);   // (+-inf clamp too)
  const float* P = prob + b * (size_t)D * hw + p;
  float s = 0.0f;
#pragma unroll
  for (int k = k0 - 1; k <= k0 + 2; ++k)
    if (k >= 0 && k < D) s += P[(size_t)k * hw];
  conf[e] = s;
}

struct Vec3 {
  double x, y, z;
};

__device__ inline Vec3 mat_vec(const Mat3& m, double x, double y, double z) {
  return {m.a[0] * x + m.a[1] * y + m.a[2] * z, m.a[3] * x + m.a[4] * y + m.a[5] * z,
          m.a[6] * x + m.a[7] * y + m.a[8] * z};
}

__device__ inline Mat3 transposed(const Mat3& m) {
  return {{m.a[0], m.a[3], m.a[6], m.a[1], m.a[4], m.a[7], m.a[2], m.a[5], m.a[8]}};
}

// The 12 doubles that take a pixel (x, y) of camera a at depth d to camera b's pixel and depth:
// p = d M (x, y, 1)^T + m with M = (K_b R_b) (R_a^T K_a^-1), m = K_b (T_b - (R_b R_a^T) T_a)   (x_cam = R x_world + T)
__device__ inline void pair_matrix(const float* __restrict__ K, const float* __restrict__ R,
                                   const float* __restrict__ T, int a, int b, double* __restrict__ o) {
  const float* Ta = T + 3 * (size_t)a;
  const float* Tb = T + 3 * (size_t)b;
  const Mat3 Ka = load_mat(K + 9 * (size_t)a), Ra = load_mat(R + 9 * (size_t)a);
  const Mat3 Kb = load_mat(K + 9 * (size_t)b), Rb = load_mat(R + 9 * (size_t)b);
  const Mat3 RaT = transposed(Ra);
  const Mat3 M = mat_mul(mat_mul(Kb, Rb), mat_mul(RaT, mat_inv(Ka)));
  const Vec3 r = mat_vec(mat_mul(Rb, RaT), (double)Ta[0], (double)Ta[1], (double)Ta[2]);
  const Vec3 m = mat_vec(Kb, (double)Tb[0] - r.x, (double)Tb[1] - r.y, (double)Tb[2] - r.z);
#pragma unroll
  for (int e = 0; e < 9; ++e) o[e] = M.a[e];
  o[9] = m.x;
  o[10] = m.y;
  o[11] = m.z;
}

// a slot's source view, or -1: the slot is empty (-1), names the view itself, or names no view at all
__device__ inline int slot_source(const int* __restrict__ pairs, int N, int S, int n, int s) {
  const int v = pairs[(size_t)n * S + s];
  return (v < 0 || v >= N || v == n) ? -1 : v;
}

// b. one thread per (view n, slot s): out[n][s] = {M, m of n -> source, M', m' of source -> n}, 24 doubles; an empty
// slot's 24 are written as zeros (never read by the consistency kernel, which tests the slot itself)
__global__ __launch_bounds__(kFilterBlock) void view_pair_matrices_kernel(const float* __restrict__ K,
                                                                          const float* __restrict__ R,
                                                                          const float* __restrict__ T,
                                                                          const int* __restrict__ pairs, int N, int S,
                                                                          double* __restrict__ out) {
  const int e = (int)(blockIdx.x * kFilterBlock + threadIdx.x);
  if (e >= N * S) return;
  const int n = e / S, s = e - n * S;
  double* o = out + (size_t)e * 24;
  const int src = slot_source(pairs, N, S, n, s);
  if (src < 0) {
#pragma unroll
    for (int k = 0; k < 24; ++k) o[k] = 0.0;
    return;
  }
  pair_matrix(K, R, T, n, src, o);
  pair_matrix(K, R, T, src, n, o + 12);
}

// c. depth [N][1][h][w]; per pixel of view n with d > 0 and per non-empty slot, in fp64: project into the source,
// blend its four taps (all inside the map and > 0), project back, and count the slot when the pixel returns within
// px_thresh and its depth within rel_thresh * d.  Every comparison is written so that a NaN fails it.
__global__ __launch_bounds__(kFilterBlock) void geometric_consistency_kernel(const float* __restrict__ depth,
                                                                             const int* __restrict__ pairs,
                                                                             const double* __restrict__ mats, int N,
                                                                             int S, int h, int w, double px2,
                                                                             double rel, int* __restrict__ count,
                                                                             float* __restrict__ avg) {
  const uint32_t hw = (uint32_t)h * (uint32_t)w;
  const size_t e = (size_t)blockIdx.x * kFilterBlock + threadIdx.x;
  if (e >= (size_t)N * hw) return;
  const int n = (int)(e / hw);
  const uint32_t p = (uint32_t)(e - (size_t)n * hw);
  const int yi = (int)(p / (uint32_t)w), xi = (int)(p - (uint32_t)yi * (uint32_t)w);
  const float df = depth[e];
  if (!(df > 0.0f)) {
    count[e] = 0;
    avg[e] = 0.0f;
    return;
  }
  const double d = (double)df, x = (double)xi, y = (double)yi;
  double sum = 0.0;
  int cnt = 0;
  for (int s = 0; s < S; ++s) {
    const int src = slot_source(pairs, N, S, n, s);
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
    const float* sp = depth + (size_t)src * hw + (size_t)((int)y0 * w + (int)x0);
    const float t00 = sp[0], t01 = sp[1], t10 = sp[w], t11 = sp[w + 1];
    if (!(t00 > 0.0f && t01 > 0.0f && t10 > 0.0f && t11 > 0.0f)) continue;
    const double fx = xs - x0, fy = ys - y0;
    const double ds = (1.0 - fy) * ((1.0 - fx) * (double)t00 + fx * (double)t01) +
                      fy * ((1.0 - fx) * (double)t10 + fx * (double)t11);
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
    sum += qz;
    ++cnt;
  }
  count[e] = cnt;
  avg[e] = (float)((d + sum) / (double)(1 + cnt));
}

// d. xyz [N][h][w][3] = R_n^T (d K_n^-1 (x, y, 1)^T - T_n), fp64, rounded once; an invalid d gives three zeros
__global__ __launch_bounds__(kFilterBlock) void backproject_kernel(const float* __restrict__ depth,
                                                                   const float* __restrict__ K,
                                                                   const float* __restrict__ R,
                                                                   const float* __restrict__ T, int N, int h, int w,
                                                                   float* __restrict__ xyz) {
  const uint32_t hw = (uint32_t)h * (uint32_t)w;
  const size_t e = (size_t)blockIdx.x * kFilterBlock + threadIdx.x;
  if (e >= (size_t)N * hw) return;
  const int n = (int)(e / hw);
  const uint32_t p = (uint32_t)(e - (size_t)n * hw);
  const int yi = (int)(p / (uint32_t)w), xi = (int)(p - (uint32_t)yi * (uint32_t)w);
  float* o = xyz + e * 3;
  const float df = depth[e];
  if (!(df > 0.0f)) {
    o[0] = 0.0f;
    o[1] = 0.0f;
    o[2] = 0.0f;
    return;
  }
  const double d = (double)df;
  const Vec3 ray = mat_vec(mat_inv(load_mat(K + 9 * (size_t)n)), (double)xi, (double)yi, 1.0);
  const float* Tn = T + 3 * (size_t)n;
  const Mat3 Rn = load_mat(R + 9 * (size_t)n);
  const double cx = d * ray.x - (double)Tn[0], cy = d * ray.y - (double)Tn[1], cz = d * ray.z - (double)Tn[2];
  o[0] = (float)(Rn.a[0] * cx + Rn.a[3] * cy + Rn.a[6] * cz);
  o[1] = (float)(Rn.a[1] * cx + Rn.a[4] * cy + Rn.a[7] * cz);
  o[2] = (float)(Rn.a[2] * cx + Rn.a[5] * cy + Rn.a[8] * cz);
}

}  // namespace

void launch_photometric_confidence(const float* prob, const float* depth, const float* d_batch, int B, int D,
                                   uint32_t hw, float* conf, hipStream_t s) {
  hipLaunchKernelGGL(photometric_confidence_kernel, filter_grid((size_t)B * hw), dim3(kFilterBlock), 0, s, prob,
                     depth, d_batch, B, D, hw, conf);
}

void launch_view_pair_matrices(const float* K, const float* R, const float* T, const int* pairs, int N, int S,
                               double* out, hipStream_t s) {
  hipLaunchKernelGGL(view_pair_matrices_kernel, filter_grid((size_t)N * (size_t)S), dim3(kFilterBlock), 0, s, K, R, T,
                     pairs, N, S, out);
}

void launch_geometric_consistency(const float* depth, const int* pairs, const double* mats, int N, int S, int h, int w,
                                  double px_thresh, double rel_thresh, int* count, float* avg, hipStream_t s) {
  hipLaunchKernelGGL(geometric_consistency_kernel, filter_grid((size_t)N * (size_t)h * (size_t)w), dim3(kFilterBlock),
                     0, s, depth, pairs, mats, N, S, h, w, px_thresh * px_thresh, rel_thresh, count, avg);
}

void launch_backproject(const float* depth, const float* K, const float* R, const float* T, int N, int h, int w,
                        float* xyz, hipStream_t s) {
  hipLaunchKernelGGL(backproject_kernel, filter_grid((size_t)N * (size_t)h * (size_t)w), dim3(kFilterBlock), 0, s,
                     depth, K, R, T, N, h, w, xyz);
}

}  // namespace mvs
