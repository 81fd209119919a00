// bn_train_bwd.hip -- the backward of the train-mode BatchNorm + ReLU sites of the regulariser under autograd
// (mvs_amd/bn_train.py; the forward is channel_ops.hip's channel_stats_* and bn_relu_*):
//   out = relu((z[box] - mean) * scale + shift), the batch statistics over ALL of z.
// Two HBM-bound passes, each in a channels-last (x[b][voxel][c]) and an NCDHW (x[b][c][voxel]) form:
//
//   reduce  ga = gy where (z - mean) * scale + shift > 0 (channel_ops.hip's expression and contraction, so the
//           mask is the forward's), 0 elsewhere; per channel S_g = sum ga and S_gz = sum ga * z over the box in
//           float64: per thread, then across the wave's lanes of equal channel, then across the workgroup's
//           waves through LDS in a fixed order, WRITTEN (no atomics) to the workgroup's own slot
//           stats[slot][0 / 1][c]; the caller adds the slots in a fixed order.  Bit-identical run to run, and
//           nothing is zeroed beforehand.  Reads gy and the box of z once.
//   apply   gz = ga * scale + g_s1 + 2 z g_s2 over ALL of z (ga = 0 outside the box), written once in z's
//           layout.  Reads z once and gy once.
//
// The box: z has extents n = (D, H, W) per sample, gy is contiguous on the index box [o, o + s) of it.  A thread
// walks its grid-stride items with carried (x, y, z, sample) coordinates: the stride's own decomposition is
// formed on the host, so the loop has no division.  Offsets are size_t: z and gy may pass 2^32 bytes.
// 16-byte accesses: always in the channels-last form (C a multiple of 4); in the NCDHW form when there is no
// box and the plane is a multiple of 4, scalar otherwise (a box row starts at any x).
#include "launchers.h"

namespace mvs {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr unsigned kBwdClBlocks = 2048;   // channels-last: at most this many workgroups (= slots of the reduce)

// a position in an [.][n0][n1][n2] grid and the step a grid stride makes in it (st[k] < n[k])
struct Walk {
  int n[3], st[3];
  size_t sb;
};

Walk make_walk(const int* n, size_t step) {
  Walk w;
  for (int k = 0; k < 3; ++k) w.n[k] = n[k];
  w.st[2] = (int)(step % (size_t)n[2]);
  step /= (size_t)n[2];
  w.st[1] = (int)(step % (size_t)n[1]);
  step /= (size_t)n[1];
  w.st[0] = (int)(step % (size_t)n[0]);
  w.sb = step / (size_t)n[0];
  return w;
}

struct Pos {
  int i[3];
  size_t b;
};

__device__ inline Pos pos_of(size_t v, const Walk& w) {
  Pos p;
  p.i[2] = (int)(v % (size_t)w.n[2]);
  v /= (size_t)w.n[2];
  p.i[1] = (int)(v % (size_t)w.n[1]);
  v /= (size_t)w.n[1];
  p.i[0] = (int)(v % (size_t)w.n[0]);
  p.b = v / (size_t)w.n[0];
  return p;
}

// one grid stride on: every coordinate gains its step and at most one carry, so one conditional subtraction each
__device__ inline void advance(Pos& p, const Walk& w) {
  int carry = 0;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    int v = p.i[k] + w.st[k] + carry;
    carry = v >= w.n[k] ? 1 : 0;
    p.i[k] = v - (carry ? w.n[k] : 0);
  }
  p.b += w.sb + (size_t)carry;
}

// the box [o, o + s) of a volume of extents n
struct Box {
  int n[3], o[3], s[3];
};

__device__ inline bool inside(const Pos& p, const Box& g) {
  return p.i[0] >= g.o[0] && p.i[0] < g.o[0] + g.s[0] && p.i[1] >= g.o[1] && p.i[1] < g.o[1] + g.s[1] &&
         p.i[2] >= g.o[2] && p.i[2] < g.o[2] + g.s[2];
}

// voxel index of the box position p (box coordinates) in the volume / of the volume position p in the box
__device__ inline size_t vol_voxel(const Pos& p, const Box& g) {
  return ((p.b * g.n[0] + (size_t)(p.i[0] + g.o[0])) * g.n[1] + (size_t)(p.i[1] + g.o[1])) * g.n[2] +
         (size_t)(p.i[2] + g.o[2]);
}
__device__ inline size_t box_voxel(const Pos& p, const Box& g) {
  return ((p.b * g.s[0] + (size_t)(p.i[0] - g.o[0])) * g.s[1] + (size_t)(p.i[1] - g.o[1])) * g.s[2] +
         (size_t)(p.i[2] - g.o[2]);
}

// gy where the forward's pre-activation is positive (bn_relu_*_kernel's expression: the same sub + fma)
__device__ inline float masked(float g, float v, float sc, float sh, float mu) {
  return (v - mu) * sc + sh > 0.0f ? g : 0.0f;
}

__device__ inline float grad_z(float ga, float v, float sc, float g1, float g22) { return ga * sc + (g1 + v * g22); }

// ---- channels-last: float4 j holds channels 4 (j % C4) .. + 3 of voxel j / C4; the grid stride is a multiple of
// C4 (C4 divides kBlock), so a thread's quad never changes ----
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_cl_kernel(
    const float4* __restrict__ z, const float4* __restrict__ gy, size_t ng4, int C4, Box g, Walk w, int whole,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mu,
    double* __restrict__ stats) {
  __shared__ double part[kWaves][64][8];
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t stride = (size_t)gridDim.x * kBlock;
  const size_t j0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const int quad = (int)(j0 % (size_t)C4);
  float a[4], b[4], m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[k] = sc[4 * quad + k];
    b[k] = sh[4 * quad + k];
    m[k] = mu[4 * quad + k];
  }
  Pos p = pos_of(j0 / (size_t)C4, w);   // (box coordinates)
  for (size_t j = j0; j < ng4; j += stride) {
    const float4 gv = gy[j];
    const float4 v = z[whole ? j : vol_voxel(p, g) * (size_t)C4 + (size_t)quad];
    const float e[4] = {v.x, v.y, v.z, v.w};
    const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double ga = (double)masked(ge[k], e[k], a[k], b[k], m[k]);
      s[k] += ga;
      q[k] += ga * (double)e[k];
    }
    if (!whole) advance(p, w);
  }
  // lanes l and l ^ o (o >= C4) hold the same quad
  for (int o = 32; o >= C4; o >>= 1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s[k] += __shfl_xor(s[k], o);
      q[k] += __shfl_xor(q[k], o);
    }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane < C4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      part[wave][lane][k] = s[k];
      part[wave][lane][4 + k] = q[k];
    }
  }
  __syncthreads();
  if (wave == 0 && lane < C4) {
    const int C = 4 * C4;
    double* st = stats + (size_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double u = part[0][lane][k], t = part[0][lane][4 + k];
#pragma unroll
      for (int v = 1; v < kWaves; ++v) {
        u += part[v][lane][k];
        t += part[v][lane][4 + k];
      }
      st[4 * lane + k] = u;
      st[C + 4 * lane + k] = t;
    }
  }
}

__global__ __launch_bounds__(kBlock) void bn_bwd_apply_cl_kernel(
    const float4* __restrict__ z, const float4* __restrict__ gy, size_t n4, int C4, Box g, Walk w, int whole,
    const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mu,
    const float* __restrict__ gs1, const float* __restrict__ gs2, float4* __restrict__ gz) {
  const size_t stride = (size_t)gridDim.x * kBlock;
  const size_t j0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const int quad = (int)(j0 % (size_t)C4);
  float a[4], b[4], m[4], g1[4], g22[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[k] = sc[4 * quad + k];
    b[k] = sh[4 * quad + k];
    m[k] = mu[4 * quad + k];
    g1[k] = gs1[4 * quad + k];
    g22[k] = 2.0f * gs2[4 * quad + k];
  }
  Pos p = pos_of(j0 / (size_t)C4, w);   // (volume coordinates)
  for (size_t j = j0; j < n4; j += stride) {
    const float4 v = z[j];
    float4 gv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (whole)
      gv = gy[j];
    else if (inside(p, g))
      gv = gy[box_voxel(p, g) * (size_t)C4 + (size_t)quad];
    gz[j] = make_float4(grad_z(masked(gv.x, v.x, a[0], b[0], m[0]), v.x, a[0], g1[0], g22[0]),
                        grad_z(masked(gv.y, v.y, a[1], b[1], m[1]), v.y, a[1], g1[1], g22[1]),
                        grad_z(masked(gv.z, v.z, a[2], b[2], m[2]), v.z, a[2], g1[2], g22[2]),
                        grad_z(masked(gv.w, v.w, a[3], b[3], m[3]), v.w, a[3], g1[3], g22[3]));
    if (!whole) advance(p, w);
  }
}

// ---- NCDHW: one (sample, channel) plane per blockIdx.y; p.b stays 0 (the walk is inside one plane) ----
// Slot = blockIdx.x * B + sample: every (slot, channel) is written by exactly one workgroup.
__global__ __launch_bounds__(kBlock) void bn_bwd_reduce_cf_kernel(
    const float* __restrict__ z, const float* __restrict__ gy, size_t plane, size_t bplane, int C, Box g, Walk w,
    int whole, const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mu,
    double* __restrict__ stats) {
  __shared__ double part[kWaves][2];
  const int c = (int)blockIdx.y % C;
  const int bi = (int)blockIdx.y / C;
  const int B = (int)gridDim.y / C;
  const float* zp = z + (size_t)blockIdx.y * plane;
  const float* gp = gy + (size_t)blockIdx.y * bplane;
  const float a = sc[c], b = sh[c], m = mu[c];
  double s = 0.0, q = 0.0;
  const size_t stride = (size_t)gridDim.x * kBlock;
  const size_t j0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (whole && (plane & 3) == 0) {
    const float4* z4 = reinterpret_cast<const float4*>(zp);
    const float4* g4 = reinterpret_cast<const float4*>(gp);
    for (size_t j = j0; j < plane / 4; j += stride) {
      const float4 v = z4[j], gv = g4[j];
      const double g0 = masked(gv.x, v.x, a, b, m), g1 = masked(gv.y, v.y, a, b, m),
                   g2 = masked(gv.z, v.z, a, b, m), g3 = masked(gv.w, v.w, a, b, m);
      s += g0 + g1 + g2 + g3;
      q += g0 * v.x + g1 * v.y + g2 * v.z + g3 * v.w;
    }
  } else {
    Pos p = pos_of(j0, w);   // (box coordinates)
    for (size_t j = j0; j < bplane; j += stride) {
      const float v = zp[whole ? j : vol_voxel(p, g)];
      const double ga = masked(gp[j], v, a, b, m);
      s += ga;
      q += ga * (double)v;
      if (!whole) advance(p, w);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    q += __shfl_xor(q, o);
  }
  const int wave = (int)threadIdx.x >> 6;
  if (((int)threadIdx.x & 63) == 0) {
    part[wave][0] = s;
    part[wave][1] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) {
      s += part[v][0];
      q += part[v][1];
    }
    double* st = stats + ((size_t)blockIdx.x * B + bi) * 2 * C;
    st[c] = s;
    st[C + c] = q;
  }
}

__global__ __launch_bounds__(kBlock) void bn_bwd_apply_cf_kernel(
    const float* __restrict__ z, const float* __restrict__ gy, size_t plane, size_t bplane, int C, Box g, Walk w,
    int whole, const float* __restrict__ sc, const float* __restrict__ sh, const float* __restrict__ mu,
    const float* __restrict__ gs1, const float* __restrict__ gs2, float* __restrict__ gz) {
  const int c = (int)blockIdx.y % C;
  const float* zp = z + (size_t)blockIdx.y * plane;
  const float* gp = gy + (size_t)blockIdx.y * bplane;
  float* op = gz + (size_t)blockIdx.y * plane;
  const float a = sc[c], b = sh[c], m = mu[c], g1 = gs1[c], g22 = 2.0f * gs2[c];
  const size_t stride = (size_t)gridDim.x * kBlock;
  const size_t j0 = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (whole && (plane & 3) == 0) {
    const float4* z4 = reinterpret_cast<const float4*>(zp);
    const float4* g4 = reinterpret_cast<const float4*>(gp);
    float4* o4 = reinterpret_cast<float4*>(op);
    for (size_t j = j0; j < plane / 4; j += stride) {
      const float4 v = z4[j], gv = g4[j];
      o4[j] = make_float4(grad_z(masked(gv.x, v.x, a, b, m), v.x, a, g1, g22),
                          grad_z(masked(gv.y, v.y, a, b, m), v.y, a, g1, g22),
                          grad_z(masked(gv.z, v.z, a, b, m), v.z, a, g1, g22),
                          grad_z(masked(gv.w, v.w, a, b, m), v.w, a, g1, g22));
    }
  } else {
    Pos p = pos_of(j0, w);   // (volume coordinates)
    for (size_t j = j0; j < plane; j += stride) {
      const float v = zp[j];
      float gv = 0.0f;
      if (whole)
        gv = gp[j];
      else if (inside(p, g))
        gv = gp[box_voxel(p, g)];
      op[j] = grad_z(masked(gv, v, a, b, m), v, a, g1, g22);
      if (!whole) advance(p, w);
    }
  }
}

unsigned grid_cl(size_t n4) {
  const size_t blocks = (n4 + kBlock - 1) / kBlock;
  return (unsigned)(blocks < kBwdClBlocks ? blocks : kBwdClBlocks);
}

// workgroups per plane: about 2048 in total, at least one per plane, none without a first item
unsigned grid_cf(size_t items, size_t planes) {
  size_t per = (2048 + planes - 1) / planes;
  const size_t need = (items + kBlock - 1) / kBlock;
  if (per > need) per = need;
  return (unsigned)(per > 0 ? per : 1);
}

size_t voxels(const int* n) { return (size_t)n[0] * (size_t)n[1] * (size_t)n[2]; }

Box make_box(const int* n, const int* o, const int* s) {
  Box g;
  for (int k = 0; k < 3; ++k) {
    g.n[k] = n[k];
    g.o[k] = o[k];
    g.s[k] = s[k];
  }
  return g;
}

bool is_whole(const int* n, const int* s) { return s[0] == n[0] && s[1] == n[1] && s[2] == n[2]; }

// items of one NCDHW plane as the kernels walk it: float4 when it is read flat and is a multiple of 4
size_t cf_items(size_t plane, bool whole) { return whole && (plane & 3) == 0 ? plane / 4 : plane; }

}  // namespace

size_t bn_relu_bwd_slots(bool channels_last, int B, int C, const int* n, const int* s) {
  if (channels_last) return grid_cl((size_t)B * voxels(s) * (size_t)(C / 4));
  return (size_t)grid_cf(cf_items(voxels(s), is_whole(n, s)), (size_t)B * C) * (size_t)B;
}

void launch_bn_relu_bwd_reduce(const float* z, const float* gy, bool channels_last, int B, int C, const int* n,
                               const int* o, const int* s, const float* sc, const float* sh, const float* mu,
                               double* stats, hipStream_t st) {
  const Box g = make_box(n, o, s);
  const int whole = is_whole(n, s) ? 1 : 0;
  if (channels_last) {
    const int C4 = C / 4;
    const size_t ng4 = (size_t)B * voxels(s) * (size_t)C4;
    const unsigned grid = grid_cl(ng4);
    const Walk w = make_walk(s, (size_t)grid * kBlock / (size_t)C4);
    hipLaunchKernelGGL(bn_bwd_reduce_cl_kernel, dim3(grid), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(z),
                       reinterpret_cast<const float4*>(gy), ng4, C4, g, w, whole, sc, sh, mu, stats);
  } else {
    const size_t plane = voxels(n), bplane = voxels(s);
    const unsigned grid = grid_cf(cf_items(bplane, whole != 0), (size_t)B * C);
    const Walk w = make_walk(s, (size_t)grid * kBlock);
    hipLaunchKernelGGL(bn_bwd_reduce_cf_kernel, dim3(grid, (unsigned)(B * C)), dim3(kBlock), 0, st, z, gy, plane,
                       bplane, C, g, w, whole, sc, sh, mu, stats);
  }
}

void launch_bn_relu_bwd_apply(const float* z, const float* gy, bool channels_last, int B, int C, const int* n,
                              const int* o, const int* s, const float* sc, const float* sh, const float* mu,
                              const float* gs1, const float* gs2, float* gz, hipStream_t st) {
  const Box g = make_box(n, o, s);
  const int whole = is_whole(n, s) ? 1 : 0;
  if (channels_last) {
    const int C4 = C / 4;
    const size_t n4 = (size_t)B * voxels(n) * (size_t)C4;
    const unsigned grid = grid_cl(n4);
    const Walk w = make_walk(n, (size_t)grid * kBlock / (size_t)C4);
    hipLaunchKernelGGL(bn_bwd_apply_cl_kernel, dim3(grid), dim3(kBlock), 0, st, reinterpret_cast<const float4*>(z),
                       reinterpret_cast<const float4*>(gy), n4, C4, g, w, whole, sc, sh, mu, gs1, gs2,
                       reinterpret_cast<float4*>(gz));
  } else {
    const size_t plane = voxels(n), bplane = voxels(s);
    const unsigned grid = grid_cf(cf_items(plane, true), (size_t)B * C);   // (bn_relu_bwd_slots of the whole volume)
    const Walk w = make_walk(n, (size_t)grid * kBlock);
    hipLaunchKernelGGL(bn_bwd_apply_cf_kernel, dim3(grid, (unsigned)(B * C)), dim3(kBlock), 0, st, z, gy, plane,
                       bplane, C, g, w, whole, sc, sh, mu, gs1, gs2, gz);
  }
}

}  // namespace mvs
