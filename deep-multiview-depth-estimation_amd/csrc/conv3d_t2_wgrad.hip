// conv3d_t2_wgrad.hip -- weight gradient of the regulariser's transposed region convolutions under autograd
// (deconv_3_0 64 -> 32 and deconv_2_0 32 -> 16, model.py:117-120: ConvTranspose3d(3, stride 2) from the M-region
// tensor to a box of the whole volume; mvs_amd/region_train.py _T2Box), on wgrad_taprow.h's plan.
//
//   dW[ci][co][t] = sum over the batch and every input voxel i of x[b][i][ci] * gy[b][2 i - crop + t][co]
//
// (terms off gy's box are 0): conv3d_s2_wgrad.hip's sum with the roles exchanged -- the COARSE-grid tensor is
// the layer's input x (CC = 64 or 32 channels), the FINE-grid tensor its output gradient gy (CF = 32 or 16), both
// channels-last: x [B][Iz][Iy][Ix][CC], gy [B][Oz][Oy][Ox][CF] (the layout autograd delivers gy in at the
// training shapes; read in place).  Per tap t a CC x CF GEMM with K = the coarse voxels.  A tile is TR coarse rows
// (flattened b, iz, iy).  The four waves:
//   (64, 32): wave = (co block of 2, ci blocks 0-1 or 2-3): 3 x 2 accumulators, every row of the tile;
//   (32, 16): wave = the rows r = kp mod 4 of the tile (KP = 4 partial sums of K), both ci blocks: 3 x 2
//             accumulators; each (chunk, kp) has a slot of its own.
// Per tile it stages
//   x:  TR x 16 voxel records of CC + 16 floats;
//   gy: the tap row's fine row (b, 2 iz - cz + tz, 2 iy - cy + ty) of each coarse row, the 34 fine voxels
//       2 x0 - cx + j along x as records of CF floats (CF = 32: + 16) in the header's parity order.
// Every record length is 16 mod 32 floats: the two K indices of a 32-lane half of an operand read (ds_read_b32:
// 32 banks per half) land on disjoint halves of the banks.  Coarse rows whose fine row is off the box are skipped
// (their products are all 0).  LDS: 69,984 B (64, 32; TR = 6) and 63,168 B (32, 16; TR = 12) per workgroup, two
// workgroups per CU.  gy's byte offsets pass 2^32 at the training shapes.
#include "launchers.h"
#include "wgrad_taprow.h"

namespace mvs {
namespace {

template <int CC, int CF>
struct TwTile {
  static_assert((CC == 64 && CF == 32) || (CC == 32 && CF == 16), "deconv_3_0 / deconv_2_0");
  static constexpr int TR = CC == 64 ? 6 : 12;      // coarse rows per tile
  static constexpr int KP = CC == 64 ? 1 : 4;       // partial sums of K per workgroup (waves that split the rows)
  static constexpr int PC = CC + 16;                // floats per staged x record
  static constexpr int PF = CF == 32 ? 48 : 16;     // floats per staged gy record
  static constexpr int CV = TR * kTapRowTX, FV = TR * kTapRowFR;
  static constexpr int SLOT = 27 * CC * CF;         // floats per partial slot
  static constexpr int LDS = (CV * PC + FV * PF) * 4 + 2 * TR * 8;
  static_assert(PC % 32 == 16 && PF % 32 == 16, "operand reads: the two K indices of a half on disjoint banks");
  static_assert(LDS <= 80 * 1024, "two workgroups per CU");
};

struct TwGeo {
  int B;
  int Iz, Iy, Ix;        // x's extent (the coarse grid)
  int Oz, Oy, Ox;        // gy's box (the fine grid)
  int cz, cy, cx;        // crop
  TapRowGeo t;           // rows: B * Iz * Iy coarse rows
};

template <int CC, int CF>
__global__ __launch_bounds__(kBlock) void conv3d_t2_wgrad_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gy,
                                                                float* __restrict__ part, TwGeo g) {
  using T = TwTile<CC, CF>;
  constexpr int TR = T::TR, KP = T::KP, PC = T::PC, PF = T::PF;
  __shared__ __attribute__((aligned(16))) float cs[T::CV * PC];
  __shared__ __attribute__((aligned(16))) float fs[T::FV * PF];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const TapRowBlock blk = taprow_block();
  // this wave's blocks: co block nb, ci blocks cb0 and cb0 + 1, the tile's rows kp, kp + KP, ...
  const int nb = KP == 1 ? (wave & 1) : 0, cb0 = KP == 1 ? (wave >> 1) * 2 : 0, kp = KP == 1 ? 0 : wave;
  // A: lane (m, kq) supplies x[voxel 4 s + kq][ci = cb * 16 + m]; B: gy[record of voxel 4 s + kq][co = nb * 16 + m]
  const int aoff = kq * PC + cb0 * 16 + m, boff = kq * PF + nb * 16 + m;

  f4v acc[3][2];
  taprow_zero(acc);
  taprow_walk<TR>(
      blk, g.t,
      [&](int R, long long& oc, long long& of) {
        const int iy = R % g.Iy, t = R / g.Iy;
        const int iz = t % g.Iz, b = t / g.Iz;
        const int fz = 2 * iz - g.cz + blk.tz, fy = 2 * iy - g.cy + blk.ty;
        oc = (long long)R * g.Ix * CC;
        if (fz >= 0 && fz < g.Oz && fy >= 0 && fy < g.Oy)
          of = (((long long)b * g.Oz + fz) * g.Oy + fy) * g.Ox * CF;   // gy[b][fz][fy][0][0]
      },
      [&](int x0, const long long* rowc, const long long* rowf) {
        taprow_stage_rows<CC, PC, TR, kTapRowTX, true>(cs, x, rowc, rowf, x0, g.Ix);
        // the tile's first fine voxel along x, 2 x0 - cx, may be negative
        taprow_stage_parity_rows<CF, PF, TR>(fs, gy, rowf, 2 * x0 - g.cx, g.Ox);
        __syncthreads();
#pragma unroll 1
        for (int r = kp; r < TR; r += KP) {
          if (rowf[r] < 0) continue;   // wave-uniform: no such row, or its fine row is off the box
          taprow_ksteps<2, 2, PC, PF>(cs + r * kTapRowTX * PC + aoff, fs + r * kTapRowFR * PF + boff, acc);
        }
      });
  // partial slot [27][ci][co]
  taprow_store_slot<CC, CF>(part + ((size_t)blk.chunk * KP + kp) * T::SLOT, blk.row_tap, cb0, 2, nb, lane, acc);
}

template <int CC, int CF>
TwGeo tw_geo(int B, const int* in, const int* crop, const int* out) {
  TwGeo g;
  g.B = B;
  g.Iz = in[0], g.Iy = in[1], g.Ix = in[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.cz = crop ? crop[0] : 0, g.cy = crop ? crop[1] : 0, g.cx = crop ? crop[2] : 0;
  g.t = taprow_geo(B * g.Iz * g.Iy, g.Ix, TwTile<CC, CF>::TR);
  return g;
}

template <int CC, int CF>
size_t tw_workspace_bytes(int B, const int* in, const int* out) {
  return taprow_workspace_bytes(tw_geo<CC, CF>(B, in, nullptr, out).t, TwTile<CC, CF>::KP, TwTile<CC, CF>::SLOT);
}

template <int CC, int CF>
void tw_launch(const float* x, const float* gy, int B, const int* in, const int* crop, const int* out, float* part,
               float* dw, hipStream_t s) {
  const TwGeo g = tw_geo<CC, CF>(B, in, crop, out);
  hipLaunchKernelGGL((conv3d_t2_wgrad_kernel<CC, CF>), taprow_grid(g.t), dim3(kBlock), 0, s, x, gy, part, g);
  launch_wgrad_reduce(part, taprow_chunks(g.t) * TwTile<CC, CF>::KP, CC, CF, dw, s);
}

}  // namespace

bool conv3d_t2_wgrad_supported(int CC, int CF) { return (CC == 64 && CF == 32) || (CC == 32 && CF == 16); }

size_t conv3d_t2_wgrad_workspace_bytes(int B, int CC, int CF, const int* in, const int* out) {
  if (CC == 64 && CF == 32) return tw_workspace_bytes<64, 32>(B, in, out);
  if (CC == 32 && CF == 16) return tw_workspace_bytes<32, 16>(B, in, out);
  return 0;
}

void launch_conv3d_t2_wgrad(const float* x, const float* gy, int B, int CC, int CF, const int* in, const int* crop,
                            const int* out, float* part, float* dw, hipStream_t s) {
  if (CC == 64 && CF == 32) tw_launch<64, 32>(x, gy, B, in, crop, out, part, dw, s);
  else if (CC == 32 && CF == 16) tw_launch<32, 16>(x, gy, B, in, crop, out, part, dw, s);
}

}  // namespace mvs
