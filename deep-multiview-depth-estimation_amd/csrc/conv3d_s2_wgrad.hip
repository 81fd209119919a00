// conv3d_s2_wgrad.hip -- weight gradient of the regulariser's stacked stride-2 region convolution under
// autograd (conv_1_0 / conv_2_0 / conv_3_0, model.py:101-107: Conv3d(32, 16 + 32 + 64, 3, stride 2) of the
// whole cost volume on an output box; mvs_amd/region_train.py _S2Box), on wgrad_taprow.h's plan.
//
//   dW[co][ci][t] = sum over the batch and every output voxel o of gy[b][o][co] * x[b][2 o - pad_lo + t][ci]
//
// (terms off the volume are 0) with x the contiguous NCDHW volume [B][32][D][H][W], read in place, and gy
// channels-last [B][Oz][Oy][Ox][112] is, per tap t, a 112 x 32 GEMM with K = the output voxels: 7 x 2
// accumulator blocks.  A workgroup's tap row is 3 x 7 x 2 MFMA blocks over its four waves: wave = (ci block, co
// blocks 0-3 or 4-6), 12 or 9 accumulators.  A tile is kSwTR output rows (flattened b, oz, oy); per tile it stages
//   gy: kSwTR x 16 voxel records of 112 floats; 112 = 48 mod 64, so the 4 voxels x 16 channels of an MFMA operand
//       read land on 64 distinct banks without padding;
//   x:  the tap row's input row (b, 2 oz - pz + tz, 2 oy - py + ty) of each output row, the 33 inputs
//       2 x0 - px + j along x, TRANSPOSED from NCDHW into voxel records of 32 + 16 floats (per channel plane
//       16-byte loads along W, four scalar LDS stores) in the header's parity order; with 48 floats per record an
//       operand read again covers 64 distinct banks.
// Output rows whose input row is off the volume are skipped (their products are all 0).  LDS: 68,560 B per
// workgroup, two workgroups per CU (137 KB of 160 KB).  Addresses into x are 64-bit (sample base + channel plane
// + row): a sample's byte offset passes 2^31 at the training shapes.
//
// This kernel keeps its tile walk, row-offset table, staging and slot store inline (the header's plan, statement
// for statement): through taprow_walk and the header's staging it measured 1.6 % slower at the training shape
// (8.05 against 7.92 ms), outside the parent's 0.3 % run-to-run spread.  It shares the header's constants, host
// geometry, K-step and reduce; a change of the walk in wgrad_taprow.h has to be repeated here.
#include "launchers.h"
#include "wgrad_taprow.h"

namespace mvs {
namespace {

constexpr int kSwCI = 32, kSwCO = 112;
constexpr int kSwTR = 5;                        // output rows per tile
constexpr int kSwPG = kSwCO, kSwPX = kSwCI + 16;   // floats per staged gy / x record
constexpr int kSwGV = kSwTR * kTapRowTX, kSwXV = kSwTR * kTapRowFR;
constexpr int kSwSlot = 27 * kSwCO * kSwCI;     // floats per partial slot
static_assert((kSwGV * kSwPG + kSwXV * kSwPX) * 4 + 2 * kSwTR * 8 <= 80 * 1024, "two workgroups per CU");

struct SwGeo {
  int B, D, H, W;        // the volume x
  int Oz, Oy, Ox;        // gy's box
  int pz, py, px;        // pad_lo
  TapRowGeo t;           // rows: B * Oz * Oy output rows
};

// the K-steps of one staged tile for a wave with NCB co blocks
template <int NCB>
__device__ __forceinline__ void sw_tile(const float* gys, const float* xs, const long long* rowx, int aoff, int boff,
                                        f4v (&acc)[3][4]) {
#pragma unroll 1
  for (int r = 0; r < kSwTR; ++r) {
    if (rowx[r] < 0) continue;   // workgroup-uniform: no such row, or its input row is off the volume
    taprow_ksteps<2, NCB, kSwPG, kSwPX>(gys + r * kTapRowTX * kSwPG + aoff, xs + r * kTapRowFR * kSwPX + boff, acc);
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

  for (int tile = chunk; tile < g.t.tiles; tile += chunks) {   // workgroup-uniform
    const int x0 = (tile % g.t.tiles_x) * kTapRowTX, row0 = (tile / g.t.tiles_x) * kSwTR;
    const int ix0 = 2 * x0 - g.px;   // the tile's first input along x (may be negative)
    __syncthreads();   // the previous tile's operand reads are done
    if (tid < kSwTR) {
      const int R = row0 + tid;
      long long og = -1, ox = -1;
      if (R < g.t.rows) {
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
      const int r = v / kTapRowTX, xi = v % kTapRowTX;
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
      float* dst = xs + (r * kTapRowFR + 2 * q) * kSwPX + ci;   // even record 2 q
      dst[0] = val[0];
      dst[kTapRowHX * kSwPX] = val[1];
      if (q < XQ - 1) {   // (j = 34, 35 are no tap of the tile)
        dst[kSwPX] = val[2];
        dst[(kTapRowHX + 1) * kSwPX] = val[3];
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

SwGeo sw_geo(int B, const int* n, const int* pad_lo, const int* out) {
  SwGeo g;
  g.B = B;
  g.D = n[0], g.H = n[1], g.W = n[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.pz = pad_lo ? pad_lo[0] : 0, g.py = pad_lo ? pad_lo[1] : 0, g.px = pad_lo ? pad_lo[2] : 0;
  g.t = taprow_geo(B * g.Oz * g.Oy, g.Ox, kSwTR);
  return g;
}

}  // namespace

size_t conv3d_s2_wgrad_workspace_bytes(int B, const int* n, const int* out) {
  return taprow_workspace_bytes(sw_geo(B, n, nullptr, out).t, 1, kSwSlot);
}

void launch_conv3d_s2_wgrad(const float* x, const float* gy, int B, const int* n, const int* pad_lo, const int* out,
                            float* part, float* dw, hipStream_t s) {
  const SwGeo g = sw_geo(B, n, pad_lo, out);
  hipLaunchKernelGGL(conv3d_s2_wgrad_kernel, taprow_grid(g.t), dim3(kBlock), 0, s, x, gy, part, g);
  launch_wgrad_reduce(part, taprow_chunks(g.t), kSwCO, kSwCI, dw, s);
}

}  // namespace mvs
