// loss.hip -- the training objective (the reference's loss.py:4-41, mvs_amd/loss.py) and the depth accuracy
// (config.py:4 ACC_THRESH) over the three depth maps gt, initial, refined [B][1][h][w], n = h * w per sample:
//
//   forward  one pass over the three maps.  Per sample, over the valid pixels (gt != 0; a NaN gt is valid):
//              n_valid, S0 = sum |gt - initial|, S1 = sum |gt - refined|          (differences and sums in float64)
//              A0 = #{|gt - initial| <= thresh * |gt|}, A1 alike for refined       (fp32 difference and product)
//            per thread, across the wave's lanes, across the workgroup's waves through LDS in a fixed order, WRITTEN
//            (no atomics) to the workgroup's own slot ws[blockIdx.x][b][5]: two float64 sums and three 64-bit
//            counts as 8-byte words.  Nothing is zeroed beforehand.
//   finish   adds the slots in slot order and writes loss0 = (float)S0 / (float)n_valid (one fp32 division, 0 / 0 =
//            NaN for a sample without a valid pixel), loss1, acc0 = A0 / n_valid, acc1 and n_valid as fp32 [B].
//   backward g_initial = -((c0[b] * m) * sgn(gt - initial)), m = 1 where gt != 0 and 0 elsewhere, g_refined alike with
//            c1: the products torch's autograd of the reference expression forms, in its order (0 * inf = NaN for a
//            sample without a valid pixel).  sgn(x) = (0 < x) - (x < 0), which is 0 for 0 and for NaN as torch.sign.
//            Every element of both gradients written once.
//
// The walk: a sample is cut into items of four consecutive elements [4 j, 4 j + 4), counted from the SAMPLE's first
// element, item j of the grid-stride walk of blockIdx.x's threads; blockIdx.y is the sample.  An item is one 16-byte
// access per map where it is whole and every map's address of it is 16-byte aligned (decided per sample), four
// bounds-checked scalar accesses otherwise (the ragged last item; every item of a misaligned sample).  Which thread
// sums which element therefore does not depend on the alignment: the results are the same bits either way.
// Offsets are size_t; n < 2^31 keeps the per-thread counts in 32 bits.
#include "launchers.h"

namespace mvs {
namespace {

constexpr int kWaves = kBlock / 64;
constexpr size_t kLossBlocks = 1024;   // at most about this many workgroups over all samples
constexpr int kFinishSamples = kBlock / 5;   // samples per workgroup of the finish kernel: five threads each

struct Sums {
  double s0, s1;
  unsigned n, a0, a1;
};

__device__ inline void add_pixel(Sums& t, float g, float x0, float x1, float thresh) {
  if (g != 0.0f) {   // (true for NaN)
    t.n += 1u;
    t.s0 += fabs((double)g - (double)x0);
    t.s1 += fabs((double)g - (double)x1);
    const float lim = thresh * fabsf(g);
    t.a0 += fabsf(g - x0) <= lim ? 1u : 0u;   // (false for a NaN difference)
    t.a1 += fabsf(g - x1) <= lim ? 1u : 0u;
  }
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

__global__ __launch_bounds__(kBlock) void masked_mae_fwd_kernel(const float* __restrict__ gt,
                                                                const float* __restrict__ x0,
                                                                const float* __restrict__ x1, size_t n, float thresh,
                                                                unsigned long long* __restrict__ ws) {
  __shared__ double part_s[kWaves][2];
  __shared__ unsigned part_c[kWaves][3];
  const size_t b = blockIdx.y, B = gridDim.y;
  const float* gp = gt + b * n;
  const float* p0 = x0 + b * n;
  const float* p1 = x1 + b * n;
  const bool vec = aligned16(gp) && aligned16(p0) && aligned16(p1);
  const size_t items = (n + 3) / 4;
  const size_t stride = (size_t)gridDim.x * kBlock;
  Sums t = {0.0, 0.0, 0u, 0u, 0u};
  for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < items; j += stride) {
    const size_t e = 4 * j;
    if (vec && e + 4 <= n) {
      const float4 g = *reinterpret_cast<const float4*>(gp + e);
      const float4 u = *reinterpret_cast<const float4*>(p0 + e);
      const float4 v = *reinterpret_cast<const float4*>(p1 + e);
      add_pixel(t, g.x, u.x, v.x, thresh);
      add_pixel(t, g.y, u.y, v.y, thresh);
      add_pixel(t, g.z, u.z, v.z, thresh);
      add_pixel(t, g.w, u.w, v.w, thresh);
    } else {
      for (size_t k = e; k < n && k < e + 4; ++k) add_pixel(t, gp[k], p0[k], p1[k], thresh);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    t.s0 += __shfl_xor(t.s0, o);
    t.s1 += __shfl_xor(t.s1, o);
    t.n += __shfl_xor(t.n, o);
    t.a0 += __shfl_xor(t.a0, o);
    t.a1 += __shfl_xor(t.a1, o);
  }
  const int wave = (int)threadIdx.x >> 6;
  if (((int)threadIdx.x & 63) == 0) {
    part_s[wave][0] = t.s0;
    part_s[wave][1] = t.s1;
    part_c[wave][0] = t.n;
    part_c[wave][1] = t.a0;
    part_c[wave][2] = t.a1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int v = 1; v < kWaves; ++v) {
      t.s0 += part_s[v][0];
      t.s1 += part_s[v][1];
      t.n += part_c[v][0];
      t.a0 += part_c[v][1];
      t.a1 += part_c[v][2];
    }
    unsigned long long* slot = ws + ((size_t)blockIdx.x * B + b) * 5;
    slot[0] = (unsigned long long)__double_as_longlong(t.s0);
    slot[1] = (unsigned long long)__double_as_longlong(t.s1);
    slot[2] = t.n;
    slot[3] = t.a0;
    slot[4] = t.a1;
  }
}

// thread 5 i + q of a workgroup adds word q of sample (first + i) over the slots, in slot order
__global__ __launch_bounds__(kBlock) void masked_mae_finish_kernel(const unsigned long long* __restrict__ ws,
                                                                   int slots, int B, float* __restrict__ loss0,
                                                                   float* __restrict__ loss1,
                                                                   float* __restrict__ acc0,
                                                                   float* __restrict__ acc1,
                                                                   float* __restrict__ n_valid) {
  __shared__ float total[kFinishSamples][5];
  const int i = (int)threadIdx.x / 5, q = (int)threadIdx.x % 5;
  const int b = (int)blockIdx.x * kFinishSamples + i;
  const bool live = i < kFinishSamples && b < B;
  if (live) {
    const unsigned long long* w = ws + (size_t)b * 5 + q;
    const size_t step = (size_t)B * 5;
    if (q < 2) {
      double s = 0.0;   // (unrolled: eight loads in flight, the adds still in slot order)
#pragma unroll 8
      for (int g = 0; g < slots; ++g) s += __longlong_as_double((long long)w[(size_t)g * step]);
      total[i][q] = (float)s;
    } else {
      unsigned long long c = 0;
#pragma unroll 8
      for (int g = 0; g < slots; ++g) c += w[(size_t)g * step];
      total[i][q] = (float)c;
    }
  }
  __syncthreads();
  if (live && q == 0) {
    const float nv = total[i][2];
    loss0[b] = total[i][0] / nv;
    loss1[b] = total[i][1] / nv;
    acc0[b] = total[i][3] / nv;
    acc1[b] = total[i][4] / nv;
    n_valid[b] = nv;
  }
}

__device__ inline float grad_pixel(float g, float x, float c) {
  const float m = g != 0.0f ? 1.0f : 0.0f;
  const float d = g - x;
  const float sg = (float)((0.0f < d) - (d < 0.0f));
  return -((c * m) * sg);
}

__global__ __launch_bounds__(kBlock) void masked_mae_bwd_kernel(const float* __restrict__ gt,
                                                                const float* __restrict__ x0,
                                                                const float* __restrict__ x1,
                                                                const float* __restrict__ c0,
                                                                const float* __restrict__ c1, size_t n,
                                                                float* __restrict__ g0, float* __restrict__ g1) {
  const size_t b = blockIdx.y;
  const float* gp = gt + b * n;
  const float* p0 = x0 + b * n;
  const float* p1 = x1 + b * n;
  float* o0 = g0 + b * n;
  float* o1 = g1 + b * n;
  const float a0 = c0[b], a1 = c1[b];
  const bool vec = aligned16(gp) && aligned16(p0) && aligned16(p1) && aligned16(o0) && aligned16(o1);
  const size_t items = (n + 3) / 4;
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t j = (size_t)blockIdx.x * kBlock + threadIdx.x; j < items; j += stride) {
    const size_t e = 4 * j;
    if (vec && e + 4 <= n) {
      const float4 g = *reinterpret_cast<const float4*>(gp + e);
      const float4 u = *reinterpret_cast<const float4*>(p0 + e);
      const float4 v = *reinterpret_cast<const float4*>(p1 + e);
      *reinterpret_cast<float4*>(o0 + e) = make_float4(grad_pixel(g.x, u.x, a0), grad_pixel(g.y, u.y, a0),
                                                       grad_pixel(g.z, u.z, a0), grad_pixel(g.w, u.w, a0));
      *reinterpret_cast<float4*>(o1 + e) = make_float4(grad_pixel(g.x, v.x, a1), grad_pixel(g.y, v.y, a1),
                                                       grad_pixel(g.z, v.z, a1), grad_pixel(g.w, v.w, a1));
    } else {
      for (size_t k = e; k < n && k < e + 4; ++k) {
        const float g = gp[k];
        o0[k] = grad_pixel(g, p0[k], a0);
        o1[k] = grad_pixel(g, p1[k], a1);
      }
    }
  }
}

}  // namespace

MaskedMaePlan masked_mae_plan(int B, size_t n) {
  const size_t items = (n + 3) / 4;
  const size_t need = (items + kBlock - 1) / kBlock;
  size_t per = (kLossBlocks + (size_t)B - 1) / (size_t)B;
  if (per > need) per = need;
  if (per < 1) per = 1;
  MaskedMaePlan p;
  p.workgroups = (int)per;
  p.passes = (int)((items + per * kBlock - 1) / (per * kBlock));
  return p;
}

void launch_masked_mae_fwd(const float* gt, const float* x0, const float* x1, int B, size_t n, float thresh,
                           float* loss0, float* loss1, float* acc0, float* acc1, float* n_valid,
                           unsigned long long* ws, hipStream_t st) {
  const int slots = masked_mae_plan(B, n).workgroups;
  hipLaunchKernelGGL(masked_mae_fwd_kernel, dim3((unsigned)slots, (unsigned)B), dim3(kBlock), 0, st, gt, x0, x1, n,
                     thresh, ws);
  hipLaunchKernelGGL(masked_mae_finish_kernel, dim3((unsigned)((B + kFinishSamples - 1) / kFinishSamples)),
                     dim3(kBlock), 0, st, ws, slots, B, loss0, loss1, acc0, acc1, n_valid);
}

void launch_masked_mae_bwd(const float* gt, const float* x0, const float* x1, const float* c0, const float* c1, int B,
                           size_t n, float* g0, float* g1, hipStream_t st) {
  const int grid = masked_mae_plan(B, n).workgroups;
  hipLaunchKernelGGL(masked_mae_bwd_kernel, dim3((unsigned)grid, (unsigned)B), dim3(kBlock), 0, st, gt, x0, x1, c0, c1,
                     n, g0, g1);
}

}  // namespace mvs
