// conv3d_s2_wgrad.hip -- weight gradient of the regulariser's stacked stride-2 region convolution under
// autograd (conv_1_0 / conv_2_0 / conv_3_0, model.py:101-107: Conv3d(32, 16 + 32 + 64, 3, stride 2) of the
// whole cost volume on an output box; mvs_amd/region_train.py _S2Box), on the f32-input matrix cores.
//
//   dW[co][ci][t] = sum over the batch and every output voxel o of gy[b][o][co] * x[b][2 o - pad_lo + t][ci]
//
// (terms off the volume are 0) with x the contiguous NCDHW volume [B][32][D][H][W], read in place, and gy
// channels-last [B][Oz][Oy][Ox][112] is, per tap t, a 112 x 32 GEMM with K = the output voxels: 7 x 2
// accumulator blocks.  As in conv3d_region_wgrad.hip the 27 taps are partitioned over workgroups by tap row
// (tz, ty) -- a workgroup owns the row's three x taps, 3 x 7 x 2 MFMA blocks over its four waves: wave =
// (ci block, co blocks 0-3 or 4-6), 12 or 9 accumulators -- and a workgroup is persistent over a K chunk: it
// walks tiles of kSwTR output rows (flattened b, oz, oy) x 16 output x-voxels and keeps the accumulators in
// registers across every tile of the chunk.  Per tile it stages in LDS, once,
//   gy: kSwTR x 16 voxel records of 112 floats (one 16-byte global load per 4 channels); 112 = 48 mod 64, so
//       the 4 voxels x 16 channels of an MFMA operand read land on 64 distinct banks without padding;
//   x:  the tap row's input row (b, 2 oz - pz + tz, 2 oy - py + ty) of each output row, the 33 inputs
//       2 x0 - px + j along x, TRANSPOSED from NCDHW into voxel records of 32 + 16 floats (per channel plane
//       16-byte loads along W, four scalar LDS stores) and laid out BY PARITY of j: 17 even then 17 odd
//       records, so the four output voxels of a K-step (inputs two apart) read adjacent records -- tap tx = 0
//       even record k, tx = 1 odd record k, tx = 2 even record k + 1 -- and with 48 floats per record an
//       operand read again covers 64 distinct banks.
// Output rows whose input row is off the volume are skipped (their products are all 0).  LDS: 68,560 B per
// workgroup, two workgroups per CU (137 KB of 160 KB).  Each wave stores its blocks into the chunk's partial
// [27][112][32] slot -- every slot entry is written exactly once per launch, none relies on a zeroed workspace
// -- and conv3d_s2_wgrad_reduce_kernel sums the slots in slot order (deterministic, no atomics).  Products and
// sums are fp32 (each MFMA step an fmaf chain).  Addresses into x are 64-bit (sample base + channel plane +
// row): a sample's byte offset passes 2^31 at the training shapes.
#include "launchers.h"
#include "packed.h"

namespace mvs {
namespace {

constexpr int kSwCI = 32, kSwCO = 112;
constexpr int kSwTX = 16;                       // output x-voxels of a tile
constexpr int kSwHX = kSwTX + 1;                // staged x records per parity (even: taps 0 and 2)
constexpr int kSwXR = 2 * kSwHX;                // staged x records per row
constexpr int kSwTR = 5;                        // output rows per tile
constexpr int kSwPG = kSwCO, kSwPX = kSwCI + 16;   // floats per staged gy / x record
constexpr int kSwGV = kSwTR * kSwTX, kSwXV = kSwTR * kSwXR;
constexpr int kSwChunks = 168;                  // K chunks: x 9 tap rows = 1512 workgroups, just under 3 rounds of
                                                // the 512 that fit 256 CUs at two per CU
constexpr int kSwSlot = 27 * kSwCO * kSwCI;     // floats per partial slot
static_assert((kSwGV * kSwPG + kSwXV * kSwPX) * 4 + 2 * kSwTR * 8 <= 80 * 1024, "two workgroups per CU");

struct SwGeo {
  int B, D, H, W;        // the volume x
  int Oz, Oy, Ox;        // gy's box
  int pz, py, px;        // pad_lo
  int rows;              // B * Oz * Oy output rows
  int tiles_x, tiles;    // x tiles per row group, tiles in all
};

// the K-steps of one staged tile for a wave with NCB co blocks
template <int NCB>
__device__ __forceinline__ void sw_tile(const float* gys, const float* xs, const long long* rowx, int aoff, int boff,
                                        f4v (&acc)[3][4]) {
#pragma unroll 1
  for (int r = 0; r < kSwTR; ++r) {
    if (rowx[r] < 0) continue;   // workgroup-uniform: no such row, or its input row is off the volume
#pragma unroll
    for (int s = 0; s < kSwTX / 4; ++s) {
      float a[NCB], bv[3];
#pragma unroll
      for (int c = 0; c < NCB; ++c) a[c] = gys[(r * kSwTX + 4 * s) * kSwPG + aoff + c * 16];
      bv[0] = xs[(r * kSwXR + 4 * s) * kSwPX + boff];
      bv[1] = xs[(r * kSwXR + kSwHX + 4 * s) * kSwPX + boff];
      bv[2] = xs[(r * kSwXR + 4 * s + 1) * kSwPX + boff];
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int c = 0; c < NCB; ++c)
          acc[tx][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv[tx], acc[tx][c], 0, 0, 0);
    }
  }
}

__global__ __launch_bounds__(kBlock) void conv3d_s2_wgrad_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gy,
                                                                float* __restrict__ part, SwGeo g) {
  constexpr int Q = kSwCO / 4;   // 16-byte chunks per gy voxel
  constexpr int XQ = 9;          // 16-byte chunks along W per staged x row and channel: inputs j = 0 .. 35 (34 kept)
  __shared__ __attribute__((aligned(16))) float gys[kSwGV * kSwPG];
  __shared__ __attribute__((aligned(16))) float xs[kSwXV * kSwPX];
  __shared__ long long rowg[kSwTR], rowx[kSwTR];   // element offsets of the tile's rows (-1: no such row)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int row_tap = (int)blockIdx.x % 9, chunk = (int)blockIdx.x / 9, chunks = (int)gridDim.x / 9;
  const int tz = row_tap / 3, ty = row_tap % 3;
  // this wave's blocks: ci block nb, co blocks cb0 .. cb0 + ncb - 1 (0-3 or 4-6)
  const int nb = wave & 1, half = wave >> 1;
  const int cb0 = half * 4, ncb = half ? 3 : 4;
  // A: lane (m, kq) supplies gy[voxel 4 s + kq][co = cb * 16 + m]; B: x[record of voxel 4 s + kq][ci = nb * 16 + m]
  const int aoff = kq * kSwPG + cb0 * 16 + m, boff = kq * kSwPX + nb * 16 + m;
  const long long plane = (long long)g.D * g.H * g.W;

  f4v acc[3][4];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[tx][c] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  for (int tile = chunk; tile < g.tiles; tile += chunks) {   // workgroup-uniform
    const int x0 = (tile % g.tiles_x) * kSwTX, row0 = (tile / g.tiles_x) * kSwTR;
    const int ix0 = 2 * x0 - g.px;   // the tile's first input along x (may be negative)
    __syncthreads();   // the previous tile's operand reads are done
    if (tid < kSwTR) {
      const int R = row0 + tid;
      long long og = -1, ox = -1;
      if (R < g.rows) {
        const int oy = R % g.Oy, t = R / g.Oy;
        const int oz = t % g.Oz, b = t / g.Oz;
        const int iz = 2 * oz - g.pz + tz, iy = 2 * oy - g.py + ty;
        og = (long long)R * g.Ox * kSwCO;
        if (iz >= 0 && iz < g.D && iy >= 0 && iy < g.H)
          ox = (long long)b * kSwCI * plane + ((long long)iz * g.H + iy) * g.W;   // x[b][0][iz][iy][0]
      }
      rowg[tid] = og;
      rowx[tid] = ox;
    }
    __syncthreads();
    // stage gy: items (voxel, 16-byte chunk), chunk fastest (coalesced channels-last loads); voxels past the
    // box read 0 (their products vanish)
    for (int e = tid; e < kSwGV * Q; e += kBlock) {
      const int c4 = e % Q, v = e / Q;
      const int r = v / kSwTX, xi = v % kSwTX;
      if (rowx[r] < 0) continue;
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (x0 + xi < g.Ox)
        val = *reinterpret_cast<const f4v*>(gy + rowg[r] + (long long)(x0 + xi) * kSwCO + 4 * c4);
      *reinterpret_cast<f4v*>(gys + v * kSwPG + 4 * c4) = val;
    }
    // stage x: items (row, channel, chunk of 4 inputs along W), chunk fastest; inputs off the row read 0;
    // input j goes to record (j & 1) * 17 + (j >> 1) of its row
    for (int e = tid; e < kSwTR * kSwCI * XQ; e += kBlock) {
      const int q = e % XQ, t = e / XQ;
      const int ci = t % kSwCI, r = t / kSwCI;
      const long long o = rowx[r];
      if (o < 0) continue;
      const float* src = x + o + (long long)ci * plane;
      const int ix = ix0 + 4 * q;
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (ix >= 0 && ix + 3 < g.W) {
        __builtin_memcpy(&val, src + ix, 16);   // (4-byte aligned: W is arbitrary)
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (ix + i >= 0 && ix + i < g.W) val[i] = src[ix + i];
      }
      float* dst = xs + (r * kSwXR + 2 * q) * kSwPX + ci;   // even record 2 q
      dst[0] = val[0];
      dst[kSwHX * kSwPX] = val[1];
      if (q < XQ - 1) {   // (j = 34, 35 are no tap of the tile)
        dst[kSwPX] = val[2];
        dst[(kSwHX + 1) * kSwPX] = val[3];
      }
    }
    __syncthreads();
    if (half == 0) sw_tile<4>(gys, xs, rowx, aoff, boff, acc);
    else sw_tile<3>(gys, xs, rowx, aoff, boff, acc);
  }
  // partial slot [27][co][ci]: acc[tx][c][i] = D[co = (cb0 + c) * 16 + 4 kq + i][ci = nb * 16 + m]
  float* slot = part + (size_t)chunk * kSwSlot;
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= ncb) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[((size_t)(row_tap * 3 + tx) * kSwCO + (cb0 + c) * 16 + 4 * kq + i) * kSwCI + nb * 16 + m] = acc[tx][c][i];
    }
}

// dW[co][ci][t] = the slots' [t][co][ci] entries summed in slot order (fixed: deterministic)
__global__ __launch_bounds__(kBlock) void conv3d_s2_wgrad_reduce_kernel(const float* __restrict__ part, int slots,
                                                                       float* __restrict__ dw) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);   // (t, co, ci): consecutive lanes, consecutive ci
  if (i >= kSwSlot) return;
  float s = 0.0f;
  for (int k = 0; k < slots; ++k) s += part[(size_t)k * kSwSlot + i];
  const int ci = i % kSwCI, co = (i / kSwCI) % kSwCO, t = i / (kSwCI * kSwCO);
  dw[((size_t)co * kSwCI + ci) * 27 + t] = s;
}

SwGeo sw_geo(int B, const int* n, const int* pad_lo, const int* out) {
  SwGeo g;
  g.B = B;
  g.D = n[0], g.H = n[1], g.W = n[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.pz = pad_lo ? pad_lo[0] : 0, g.py = pad_lo ? pad_lo[1] : 0, g.px = pad_lo ? pad_lo[2] : 0;
  g.rows = B * g.Oz * g.Oy;
  g.tiles_x = (g.Ox + kSwTX - 1) / kSwTX;
  g.tiles = g.tiles_x * ((g.rows + kSwTR - 1) / kSwTR);
  return g;
}

int sw_slots(const SwGeo& g) { return g.tiles < kSwChunks ? g.tiles : kSwChunks; }

}  // namespace

size_t conv3d_s2_wgrad_workspace_bytes(int B, const int* n, const int* out) {
  return (size_t)sw_slots(sw_geo(B, n, nullptr, out)) * kSwSlot * sizeof(float);
}

void launch_conv3d_s2_wgrad(const float* x, const float* gy, int B, const int* n, const int* pad_lo, const int* out,
                            float* part, float* dw, hipStream_t s) {
  const SwGeo g = sw_geo(B, n, pad_lo, out);
  const int slots = sw_slots(g);
  hipLaunchKernelGGL(conv3d_s2_wgrad_kernel, dim3(9u * (unsigned)slots), dim3(kBlock), 0, s, x, gy, part, g);
  hipLaunchKernelGGL(conv3d_s2_wgrad_reduce_kernel, dim3((kSwSlot + kBlock - 1) / kBlock), dim3(kBlock), 0, s, part,
                     slots, dw);
}

}  // namespace mvs
