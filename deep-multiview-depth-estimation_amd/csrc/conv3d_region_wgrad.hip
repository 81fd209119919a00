// conv3d_region_wgrad.hip -- weight gradient of the regulariser's stride-1 region convolutions under
// autograd (conv_1_1 / conv_2_1 / conv_3_1, model.py:108-113: Conv3d(C, C, 3) on the zero-padded crop,
// C = 16 / 32 / 64; mvs_amd/region_train.py _S1Valid), on wgrad_taprow.h's plan.
//
//   dW[co][ci][t] = sum over the batch and every output voxel o of gy[b][o][co] * x[b][o + t][ci]
//
// with both operands channels-last (x [B][Lz][Ly][Lx][C] the padded crop, gy [B][Lz-2][Ly-2][Lx-2][C])
// is, per tap t, a C x C GEMM with K = the output voxels: A = gy read as [voxel][co], B = x read as
// [voxel + t][ci].  A workgroup's tap row is 3 x (C/16)^2 MFMA blocks over its four waves
//   C = 64: wave = ci block, every co block (12 accumulators per wave)
//   C = 32: wave = (ci block, co block)      (3 accumulators)
//   C = 16: one block per tap; the waves split the tile's rows (K) four ways (3 accumulators; KP = 4 slots)
// and a tile is TR output rows: it stages the tile's gy (TR x 16 voxels) and its tap row's x (TR x 18 voxels:
// the three x taps' halo); voxel records are padded to C + 16 floats for C >= 32, so the 4 voxels x 16 channels
// of an MFMA operand read land on 64 distinct banks.
#include "launchers.h"
#include "wgrad_taprow.h"

namespace mvs {
namespace {

constexpr int kRwPX = kTapRowTX + 2;   // x-voxels of a tile's x rows

template <int C>
struct RwTile {
  static constexpr int TR = C == 64 ? 6 : (C == 32 ? 10 : 28);   // output rows per tile
  static constexpr int P = C == 16 ? 16 : C + 16;                // floats per staged voxel record
  static constexpr int NB = C / 16;                              // ci (= co) blocks
  static constexpr int KP = C == 16 ? 4 : 1;                     // K parts (waves splitting the rows)
  static constexpr int NCB = C == 64 ? 4 : 1;                    // co blocks per wave
  static constexpr int GV = TR * kTapRowTX, XV = TR * kRwPX;     // staged voxels of gy / x
  static constexpr int LDS = (GV + XV) * P * 4;                  // 60,928 / 65,280 / 65,280 B
};

struct RwGeo {
  int B, Lz, Ly, Lx;     // the padded crop x
  int Oz, Oy, Ox;        // gy: L - 2
  TapRowGeo t;           // rows: B * Oz * Oy output rows
};

template <int C>
__global__ __launch_bounds__(kBlock) void conv3d_region_wgrad_kernel(const float* __restrict__ x,
                                                                    const float* __restrict__ gy,
                                                                    float* __restrict__ part, RwGeo g) {
  using T = RwTile<C>;
  __shared__ __attribute__((aligned(16))) float gys[T::GV * T::P];
  __shared__ __attribute__((aligned(16))) float xs[T::XV * T::P];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const TapRowBlock blk = taprow_block();
  // this wave's blocks: ci block nb, co blocks cb0 .. cb0 + NCB - 1, tile rows r0 .. r0 + RW - 1
  const int nb = wave % T::NB, q = wave / T::NB;
  const int cb0 = C == 32 ? q : 0, kpart = C == 16 ? q : 0;
  constexpr int RW = T::TR / T::KP;
  const int r0 = kpart * RW;
  // A: lane (m, kq) supplies gy[voxel 4 s + kq][co = cb * 16 + m]; B: x[voxel 4 s + kq + tx][ci = nb * 16 + m]
  const int aoff = kq * T::P + cb0 * 16 + m, boff = kq * T::P + nb * 16 + m;

  f4v acc[3][T::NCB];
  taprow_zero(acc);
  taprow_walk<T::TR>(
      blk, g.t,
      [&](int R, long long& og, long long& ox) {
        const int y = R % g.Oy, t = R / g.Oy;
        const int z = t % g.Oz, b = t / g.Oz;
        og = (long long)R * g.Ox * C;
        ox = ((((long long)b * g.Lz + z + blk.tz) * g.Ly + y + blk.ty) * g.Lx) * C;
      },
      [&](int x0, const long long* rowg, const long long* rowx) {
        taprow_stage_rows<C, T::P, T::TR, kTapRowTX, false>(gys, gy, rowg, rowg, x0, g.Ox);
        taprow_stage_rows<C, T::P, T::TR, kRwPX, false>(xs, x, rowx, rowx, x0, g.Lx);
        __syncthreads();
#pragma unroll 2
        for (int r = r0; r < r0 + RW; ++r)
          taprow_ksteps<1, T::NCB, T::P, T::P>(gys + r * kTapRowTX * T::P + aoff, xs + r * kRwPX * T::P + boff, acc);
      });
  // partial slot [27][co][ci]
  taprow_store_slot<C, C>(part + (size_t)(blk.chunk * T::KP + kpart) * 27 * C * C, blk.row_tap, cb0, T::NCB, nb, lane,
                          acc);
}

template <int C>
RwGeo rw_geo(int B, const int* L) {
  RwGeo g;
  g.B = B;
  g.Lz = L[0], g.Ly = L[1], g.Lx = L[2];
  g.Oz = L[0] - 2, g.Oy = L[1] - 2, g.Ox = L[2] - 2;
  g.t = taprow_geo(B * g.Oz * g.Oy, g.Ox, RwTile<C>::TR);
  return g;
}

template <int C>
void rw_launch(const float* x, const float* gy, int B, const int* L, float* part, float* dw, hipStream_t s) {
  const RwGeo g = rw_geo<C>(B, L);
  hipLaunchKernelGGL((conv3d_region_wgrad_kernel<C>), taprow_grid(g.t), dim3(kBlock), 0, s, x, gy, part, g);
  launch_wgrad_reduce(part, taprow_chunks(g.t) * RwTile<C>::KP, C, C, dw, s);
}

template <int C>
size_t rw_workspace_bytes(int B, const int* L) {
  return taprow_workspace_bytes(rw_geo<C>(B, L).t, RwTile<C>::KP, 27 * C * C);
}

}  // namespace

bool conv3d_region_wgrad_supported(int C) { return C == 16 || C == 32 || C == 64; }

size_t conv3d_region_wgrad_workspace_bytes(int B, int C, const int* L) {
  return C == 16 ? rw_workspace_bytes<16>(B, L) : (C == 32 ? rw_workspace_bytes<32>(B, L) : rw_workspace_bytes<64>(B, L));
}

void launch_conv3d_region_wgrad(const float* x, const float* gy, int B, int C, const int* L, float* part, float* dw,
                                hipStream_t s) {
  if (C == 16) rw_launch<16>(x, gy, B, L, part, dw, s);
  else if (C == 32) rw_launch<32>(x, gy, B, L, part, dw, s);
  else rw_launch<64>(x, gy, B, L, part, dw, s);
}

}  // namespace mvs
