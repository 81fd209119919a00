// conv3d_region_wgrad.hip -- weight gradient of the regulariser's stride-1 region convolutions under
// autograd (conv_1_1 / conv_2_1 / conv_3_1, model.py:108-113: Conv3d(C, C, 3) on the zero-padded crop,
// C = 16 / 32 / 64; mvs_amd/region_train.py _S1Valid), on the f32-input matrix cores.
//
//   dW[co][ci][t] = sum over the batch and every output voxel o of gy[b][o][co] * x[b][o + t][ci]
//
// with both operands channels-last (x [B][Lz][Ly][Lx][C] the padded crop, gy [B][Lz-2][Ly-2][Lx-2][C])
// is, per tap t, a C x C GEMM with K = the output voxels: A = gy read as [voxel][co], B = x read as
// [voxel + t][ci].  The 27 C x C accumulator blocks are partitioned over workgroups by tap row (tz, ty):
// a workgroup owns the row's three x taps, 3 x (C/16)^2 MFMA blocks over its four waves
//   C = 64: wave = ci block, every co block (12 accumulators per wave)
//   C = 32: wave = (ci block, co block)      (3 accumulators)
//   C = 16: one block per tap; the waves split the tile's rows (K) four ways (3 accumulators)
// and is persistent over a K chunk: it walks tiles of TR output rows (flattened b, z, y) x 16 x-voxels,
// stages the tile's gy (TR x 16 voxels) and its tap row's x (TR x 18 voxels: the three x taps' halo) in
// LDS once (one 16-byte global load per 4 channels; voxel records padded to C + 16 floats for C >= 32, so
// the 4 voxels x 16 channels of an MFMA operand read land on 64 distinct banks), and runs the tile's
// K-steps of 4 consecutive x-voxels as v_mfma_f32_16x16x4_f32, the accumulators in registers across
// every tile of the chunk.  Each wave stores its blocks into the chunk's partial [27][C][C] slot -- every
// slot entry is written exactly once per launch, none relies on a zeroed workspace -- and
// conv3d_region_wgrad_reduce_kernel sums the slots in slot order (deterministic, no atomics).  Products
// and sums are fp32 (each MFMA step an fmaf chain).
#include "launchers.h"
#include "packed.h"

namespace mvs {
namespace {

constexpr int kRwTX = 16, kRwPX = kRwTX + 2;   // x-voxels of a tile's gy rows / x rows
constexpr int kRwChunks = 168;                 // K chunks: x 9 tap rows = 1512 workgroups, just under 3 rounds of
                                               // the 512 that fit 256 CUs at two (<= 64 KB of LDS) per CU

template <int C>
struct RwTile {
  static constexpr int TR = C == 64 ? 6 : (C == 32 ? 10 : 28);   // output rows per tile
  static constexpr int P = C == 16 ? 16 : C + 16;                // floats per staged voxel record
  static constexpr int NB = C / 16;                              // ci (= co) blocks
  static constexpr int KP = C == 16 ? 4 : 1;                     // K parts (waves splitting the rows)
  static constexpr int NCB = C == 64 ? 4 : 1;                    // co blocks per wave
  static constexpr int GV = TR * kRwTX, XV = TR * kRwPX;         // staged voxels of gy / x
  static constexpr int LDS = (GV + XV) * P * 4;                  // 60,928 / 65,280 / 65,280 B
};

struct RwGeo {
  int B, Lz, Ly, Lx;     // the padded crop x
  int Oz, Oy, Ox;        // gy: L - 2
  int rows;              // B * Oz * Oy output rows
  int tiles_x, tiles;    // x tiles per row group, tiles in all
};

template <int C>
__global__ __launch_bounds__(kBlock) void conv3d_region_wgrad_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ gy,
                                                                    float* __restrict__ part, RwGeo g) {
  using T = RwTile<C>;
  constexpr int Q = C / 4;   // 16-byte chunks per voxel
  __shared__ __attribute__((aligned(16))) float gys[T::GV * T::P];
  __shared__ __attribute__((aligned(16))) float xs[T::XV * T::P];
  __shared__ long long rowg[T::TR], rowx[T::TR];   // element offsets of the tile's rows (-1: no such row)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int row_tap = (int)blockIdx.x % 9, chunk = (int)blockIdx.x / 9, chunks = (int)gridDim.x / 9;
  const int tz = row_tap / 3, ty = row_tap % 3;
  // this wave's blocks: ci block nb, co blocks cb0 .. cb0 + NCB - 1, tile rows r0 .. r0 + RW - 1
  const int nb = wave % T::NB, q = wave / T::NB;
  const int cb0 = C == 32 ? q : 0, kpart = C == 16 ? q : 0;
  constexpr int RW = T::TR / T::KP;
  const int r0 = kpart * RW;
  // A: lane (m, kq) supplies gy[voxel 4 s + kq][co = cb * 16 + m]; B: x[voxel 4 s + kq + tx][ci = nb * 16 + m]
  const int aoff = kq * T::P + cb0 * 16 + m, boff = kq * T::P + nb * 16 + m;

  f4v acc[3][T::NCB];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < T::NCB; ++c) acc[tx][c] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  for (int tile = chunk; tile < g.tiles; tile += chunks) {   // workgroup-uniform
    const int x0 = (tile % g.tiles_x) * kRwTX, row0 = (tile / g.tiles_x) * T::TR;
    __syncthreads();   // the previous tile's operand reads are done
    if (tid < T::TR) {
      const int R = row0 + tid;
      long long og = -1, ox = -1;
      if (R < g.rows) {
        const int y = R % g.Oy, t = R / g.Oy;
        const int z = t % g.Oz, b = t / g.Oz;
        og = (long long)R * g.Ox * C;
        ox = ((((long long)b * g.Lz + z + tz) * g.Ly + y + ty) * g.Lx) * C;
      }
      rowg[tid] = og;
      rowx[tid] = ox;
    }
    __syncthreads();
    // stage: items (voxel, 16-byte chunk), chunk fastest (coalesced channels-last loads); voxels past the
    // box read 0 (their products vanish)
    for (int e = tid; e < T::GV * Q; e += kBlock) {
      const int c4 = e % Q, v = e / Q;
      const int r = v / kRwTX, xi = v % kRwTX;
      const long long o = rowg[r];
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (o >= 0 && x0 + xi < g.Ox) val = *reinterpret_cast<const f4v*>(gy + o + (long long)(x0 + xi) * C + 4 * c4);
      *reinterpret_cast<f4v*>(gys + v * T::P + 4 * c4) = val;
    }
    for (int e = tid; e < T::XV * Q; e += kBlock) {
      const int c4 = e % Q, v = e / Q;
      const int r = v / kRwPX, xi = v % kRwPX;
      const long long o = rowx[r];
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (o >= 0 && x0 + xi < g.Lx) val = *reinterpret_cast<const f4v*>(x + o + (long long)(x0 + xi) * C + 4 * c4);
      *reinterpret_cast<f4v*>(xs + v * T::P + 4 * c4) = val;
    }
    __syncthreads();
#pragma unroll 2
    for (int r = r0; r < r0 + RW; ++r) {
#pragma unroll
      for (int s = 0; s < kRwTX / 4; ++s) {
        float a[T::NCB], bv[3];
#pragma unroll
        for (int c = 0; c < T::NCB; ++c) a[c] = gys[(r * kRwTX + 4 * s) * T::P + aoff + c * 16];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) bv[tx] = xs[(r * kRwPX + 4 * s + tx) * T::P + boff];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
          for (int c = 0; c < T::NCB; ++c)
            acc[tx][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv[tx], acc[tx][c], 0, 0, 0);
      }
    }
  }
  // partial slot [27][co][ci]: acc[tx][c][i] = D[co = (cb0 + c) * 16 + 4 kq + i][ci = nb * 16 + m]
  float* slot = part + (size_t)(chunk * T::KP + kpart) * 27 * C * C;
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < T::NCB; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[((size_t)(row_tap * 3 + tx) * C + (cb0 + c) * 16 + 4 * kq + i) * C + nb * 16 + m] = acc[tx][c][i];
}

// dW[co][ci][t] = the slots' [t][co][ci] entries summed in slot order (fixed: deterministic)
__global__ __launch_bounds__(kBlock) void conv3d_region_wgrad_reduce_kernel(const float* __restrict__ part,
                                                                           int slots, int C,
                                                                           float* __restrict__ dw) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);   // (t, co, ci): consecutive lanes, consecutive ci
  const int n = 27 * C * C;
  if (i >= n) return;
  float s = 0.0f;
  for (int k = 0; k < slots; ++k) s += part[(size_t)k * n + i];
  const int ci = i % C, co = (i / C) % C, t = i / (C * C);
  dw[((size_t)co * C + ci) * 27 + t] = s;
}

template <int C>
RwGeo rw_geo(int B, const int* L) {
  RwGeo g;
  g.B = B;
  g.Lz = L[0], g.Ly = L[1], g.Lx = L[2];
  g.Oz = L[0] - 2, g.Oy = L[1] - 2, g.Ox = L[2] - 2;
  g.rows = B * g.Oz * g.Oy;
  g.tiles_x = (g.Ox + kRwTX - 1) / kRwTX;
  g.tiles = g.tiles_x * ((g.rows + RwTile<C>::TR - 1) / RwTile<C>::TR);
  return g;
}

template <int C>
int rw_slots(const RwGeo& g) {
  return (g.tiles < kRwChunks ? g.tiles : kRwChunks) * RwTile<C>::KP;
}

template <int C>
void rw_launch(const float* x, const float* gy, int B, const int* L, float* part, float* dw, hipStream_t s) {
  const RwGeo g = rw_geo<C>(B, L);
  const int slots = rw_slots<C>(g);
  hipLaunchKernelGGL((conv3d_region_wgrad_kernel<C>), dim3(9u * (unsigned)(slots / RwTile<C>::KP)), dim3(kBlock), 0,
                     s, x, gy, part, g);
  const int n = 27 * C * C;
  hipLaunchKernelGGL(conv3d_region_wgrad_reduce_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, part,
                     slots, C, dw);
}

}  // namespace

bool conv3d_region_wgrad_supported(int C) { return C == 16 || C == 32 || C == 64; }

size_t conv3d_region_wgrad_workspace_bytes(int B, int C, const int* L) {
  const int slots = C == 16 ? rw_slots<16>(rw_geo<16>(B, L))
                            : (C == 32 ? rw_slots<32>(rw_geo<32>(B, L)) : rw_slots<64>(rw_geo<64>(B, L)));
  return (size_t)slots * 27 * C * C * sizeof(float);
}

void launch_conv3d_region_wgrad(const float* x, const float* gy, int B, int C, const int* L, float* part, float* dw,
                                hipStream_t s) {
  if (C == 16) rw_launch<16>(x, gy, B, L, part, dw, s);
  else if (C == 32) rw_launch<32>(x, gy, B, L, part, dw, s);
  else rw_launch<64>(x, gy, B, L, part, dw, s);
}

}  // namespace mvs
