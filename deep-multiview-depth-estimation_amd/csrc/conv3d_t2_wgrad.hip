// conv3d_t2_wgrad.hip -- weight gradient of the regulariser's transposed region convolutions under autograd
// (deconv_3_0 64 -> 32 and deconv_2_0 32 -> 16, model.py:117-120: ConvTranspose3d(3, stride 2) from the M-region
// tensor to a box of the whole volume; mvs_amd/region_train.py _T2Box), on the f32-input matrix cores.
//
//   dW[ci][co][t] = sum over the batch and every input voxel i of x[b][i][ci] * gy[b][2 i - crop + t][co]
//
// (terms off gy's box are 0): conv3d_s2_wgrad.hip's sum with the roles exchanged -- the COARSE-grid tensor is
// the layer's input x (CC = 64 or 32 channels), the FINE-grid tensor its output gradient gy (CF = 32 or 16), both
// channels-last: x [B][Iz][Iy][Ix][CC], gy [B][Oz][Oy][Ox][CF] (the layout autograd delivers gy in at the
// training shapes; read in place).  Per tap t a CC x CF GEMM with K = the coarse voxels.  As there, the 27 taps
// are partitioned over workgroups by tap row (tz, ty) -- a workgroup owns the row's three x taps -- and a
// workgroup is persistent over a K chunk: it walks tiles of TR coarse rows (flattened b, iz, iy) x 16 coarse
// x-voxels and keeps the accumulators in registers across every tile of the chunk.  The four waves:
//   (64, 32): wave = (co block of 2, ci blocks 0-1 or 2-3): 3 x 2 accumulators, every row of the tile;
//   (32, 16): wave = the rows r = kp mod 4 of the tile (KP = 4 partial sums of K), both ci blocks: 3 x 2
//             accumulators; each (chunk, kp) has a slot of its own.
// Per tile it stages in LDS, once,
//   x:  TR x 16 voxel records of CC + 16 floats (one 16-byte global load per 4 channels);
//   gy: the tap row's fine row (b, 2 iz - cz + tz, 2 iy - cy + ty) of each coarse row, the 34 fine voxels
//       2 x0 - cx + j along x as records of CF floats (CF = 32: + 16) laid out BY PARITY of j: 17 even then 17
//       odd records, so the four coarse voxels of a K-step (fine voxels two apart) read adjacent records -- tap
//       tx = 0 even record k, tx = 1 odd record k, tx = 2 even record k + 1.
// Every record length is 16 mod 32 floats: the two K indices of a 32-lane half of an operand read (ds_read_b32:
// 32 banks per half) land on disjoint halves of the banks.  Coarse rows whose fine row is off the box are skipped
// (their products are all 0).  LDS: 69,984 B (64, 32; TR = 6) and 63,168 B (32, 16; TR = 12) per workgroup, two
// workgroups per CU.  Each wave stores its blocks into its partial [27][CC][CF] slot -- every slot entry is
// written exactly once per launch, none relies on a zeroed workspace -- and conv3d_t2_wgrad_reduce_kernel sums
// the slots in slot order (deterministic, no atomics).  Products and sums are fp32 (each MFMA step an fmaf
// chain).  Sample and row addresses are 64-bit: gy's byte offsets pass 2^32 at the training shapes.
#include "launchers.h"
#include "packed.h"

namespace mvs {
namespace {

constexpr int kTwTX = 16;               // coarse x-voxels of a tile
constexpr int kTwHX = kTwTX + 1;        // staged fine records per parity (even: taps 0 and 2)
constexpr int kTwFR = 2 * kTwHX;        // staged fine records per row
constexpr int kTwChunks = 168;          // K chunks: x 9 tap rows = 1512 workgroups, just under 3 rounds of the 512
                                        // that fit 256 CUs at two per CU

template <int CC, int CF>
struct TwTile {
  static_assert((CC == 64 && CF == 32) || (CC == 32 && CF == 16), "deconv_3_0 / deconv_2_0");
  static constexpr int TR = CC == 64 ? 6 : 12;      // coarse rows per tile
  static constexpr int KP = CC == 64 ? 1 : 4;       // partial sums of K per workgroup (waves that split the rows)
  static constexpr int PC = CC + 16;                // floats per staged x record
  static constexpr int PF = CF == 32 ? 48 : 16;     // floats per staged gy record
  static constexpr int CV = TR * kTwTX, FV = TR * kTwFR;
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
  int rows;              // B * Iz * Iy coarse rows
  int tiles_x, tiles;    // x tiles per row group, tiles in all
};

template <int CC, int CF>
__global__ __launch_bounds__(kBlock) void conv3d_t2_wgrad_kernel(const float* __restrict__ x,
                                                                const float* __restrict__ gy,
                                                                float* __restrict__ part, TwGeo g) {
  using T = TwTile<CC, CF>;
  constexpr int TR = T::TR, KP = T::KP, PC = T::PC, PF = T::PF;
  constexpr int QC = CC / 4, QF = CF / 4;   // 16-byte chunks per voxel
  __shared__ __attribute__((aligned(16))) float cs[T::CV * PC];
  __shared__ __attribute__((aligned(16))) float fs[T::FV * PF];
  __shared__ long long rowc[TR], rowf[TR];   // element offsets of the tile's rows (-1: no such row)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const int row_tap = (int)blockIdx.x % 9, chunk = (int)blockIdx.x / 9, chunks = (int)gridDim.x / 9;
  const int tz = row_tap / 3, ty = row_tap % 3;
  // this wave's blocks: co block nb, ci blocks cb0 and cb0 + 1, the tile's rows kp, kp + KP, ...
  const int nb = KP == 1 ? (wave & 1) : 0, cb0 = KP == 1 ? (wave >> 1) * 2 : 0, kp = KP == 1 ? 0 : wave;
  // A: lane (m, kq) supplies x[voxel 4 s + kq][ci = cb * 16 + m]; B: gy[record of voxel 4 s + kq][co = nb * 16 + m]
  const int aoff = kq * PC + cb0 * 16 + m, boff = kq * PF + nb * 16 + m;

  f4v acc[3][2];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[tx][c] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  for (int tile = chunk; tile < g.tiles; tile += chunks) {   // workgroup-uniform
    const int x0 = (tile % g.tiles_x) * kTwTX, row0 = (tile / g.tiles_x) * TR;
    const int fx0 = 2 * x0 - g.cx;   // the tile's first fine voxel along x (may be negative)
    __syncthreads();   // the previous tile's operand reads are done
    if (tid < TR) {
      const int R = row0 + tid;
      long long oc = -1, of = -1;
      if (R < g.rows) {
        const int iy = R % g.Iy, t = R / g.Iy;
        const int iz = t % g.Iz, b = t / g.Iz;
        const int fz = 2 * iz - g.cz + tz, fy = 2 * iy - g.cy + ty;
        oc = (long long)R * g.Ix * CC;
        if (fz >= 0 && fz < g.Oz && fy >= 0 && fy < g.Oy)
          of = (((long long)b * g.Oz + fz) * g.Oy + fy) * g.Ox * CF;   // gy[b][fz][fy][0][0]
      }
      rowc[tid] = oc;
      rowf[tid] = of;
    }
    __syncthreads();
    // stage x: items (voxel, 16-byte chunk), chunk fastest (coalesced channels-last loads); voxels past the
    // extent read 0 (their products vanish)
    for (int e = tid; e < T::CV * QC; e += kBlock) {
      const int c4 = e % QC, v = e / QC;
      const int r = v / kTwTX, xi = v % kTwTX;
      if (rowf[r] < 0) continue;
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (x0 + xi < g.Ix) val = *reinterpret_cast<const f4v*>(x + rowc[r] + (long long)(x0 + xi) * CC + 4 * c4);
      *reinterpret_cast<f4v*>(cs + v * PC + 4 * c4) = val;
    }
    // stage gy: items (row, fine voxel j, chunk), chunk fastest; voxels off the row read 0; fine voxel j goes
    // to record (j & 1) * 17 + (j >> 1) of its row
    for (int e = tid; e < TR * kTwFR * QF; e += kBlock) {
      const int c4 = e % QF, t = e / QF;
      const int j = t % kTwFR, r = t / kTwFR;
      const long long o = rowf[r];
      if (o < 0) continue;
      const int fx = fx0 + j;
      f4v val{0.0f, 0.0f, 0.0f, 0.0f};
      if (fx >= 0 && fx < g.Ox) val = *reinterpret_cast<const f4v*>(gy + o + (long long)fx * CF + 4 * c4);
      *reinterpret_cast<f4v*>(fs + (r * kTwFR + (j & 1) * kTwHX + (j >> 1)) * PF + 4 * c4) = val;
    }
    __syncthreads();
    // the K-steps of the staged tile
#pragma unroll 1
    for (int r = kp; r < TR; r += KP) {
      if (rowf[r] < 0) continue;   // wave-uniform: no such row, or its fine row is off the box
#pragma unroll
      for (int s = 0; s < kTwTX / 4; ++s) {
        float a[2], bv[3];
#pragma unroll
        for (int c = 0; c < 2; ++c) a[c] = cs[(r * kTwTX + 4 * s) * PC + aoff + c * 16];
        bv[0] = fs[(r * kTwFR + 4 * s) * PF + boff];
        bv[1] = fs[(r * kTwFR + kTwHX + 4 * s) * PF + boff];
        bv[2] = fs[(r * kTwFR + 4 * s + 1) * PF + boff];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx)
#pragma unroll
          for (int c = 0; c < 2; ++c)
            acc[tx][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], bv[tx], acc[tx][c], 0, 0, 0);
      }
    }
  }
  // partial slot [27][ci][co]: acc[tx][c][i] = D[ci = (cb0 + c) * 16 + 4 kq + i][co = nb * 16 + m]
  float* slot = part + ((size_t)chunk * KP + kp) * T::SLOT;
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[((size_t)(row_tap * 3 + tx) * CC + (cb0 + c) * 16 + 4 * kq + i) * CF + nb * 16 + m] = acc[tx][c][i];
}

// dW[ci][co][t] = the slots' [t][ci][co] entries summed in slot order (fixed: deterministic)
template <int CC, int CF>
__global__ __launch_bounds__(kBlock) void conv3d_t2_wgrad_reduce_kernel(const float* __restrict__ part, int slots,
                                                                       float* __restrict__ dw) {
  constexpr int SLOT = TwTile<CC, CF>::SLOT;
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);   // (t, ci, co): consecutive lanes, consecutive co
  if (i >= SLOT) return;
  float s = 0.0f;
  for (int k = 0; k < slots; ++k) s += part[(size_t)k * SLOT + i];
  const int co = i % CF, ci = (i / CF) % CC, t = i / (CF * CC);
  dw[((size_t)ci * CF + co) * 27 + t] = s;
}

template <int CC, int CF>
TwGeo tw_geo(int B, const int* in, const int* crop, const int* out) {
  TwGeo g;
  g.B = B;
  g.Iz = in[0], g.Iy = in[1], g.Ix = in[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.cz = crop ? crop[0] : 0, g.cy = crop ? crop[1] : 0, g.cx = crop ? crop[2] : 0;
  g.rows = B * g.Iz * g.Iy;
  g.tiles_x = (g.Ix + kTwTX - 1) / kTwTX;
  g.tiles = g.tiles_x * ((g.rows + TwTile<CC, CF>::TR - 1) / TwTile<CC, CF>::TR);
  return g;
}

inline int tw_chunks(const TwGeo& g) { return g.tiles < kTwChunks ? g.tiles : kTwChunks; }

template <int CC, int CF>
void tw_launch(const float* x, const float* gy, int B, const int* in, const int* crop, const int* out, float* part,
               float* dw, hipStream_t s) {
  using T = TwTile<CC, CF>;
  const TwGeo g = tw_geo<CC, CF>(B, in, crop, out);
  const int chunks = tw_chunks(g);
  hipLaunchKernelGGL((conv3d_t2_wgrad_kernel<CC, CF>), dim3(9u * (unsigned)chunks), dim3(kBlock), 0, s, x, gy, part, g);
  hipLaunchKernelGGL((conv3d_t2_wgrad_reduce_kernel<CC, CF>), dim3((T::SLOT + kBlock - 1) / kBlock), dim3(kBlock), 0, s,
                     part, chunks * T::KP, dw);
}

}  // namespace

bool conv3d_t2_wgrad_supported(int CC, int CF) { return (CC == 64 && CF == 32) || (CC == 32 && CF == 16); }

size_t conv3d_t2_wgrad_workspace_bytes(int B, int CC, int CF, const int* in, const int* out) {
  if (CC == 64 && CF == 32)
    return (size_t)tw_chunks(tw_geo<64, 32>(B, in, nullptr, out)) * TwTile<64, 32>::KP * TwTile<64, 32>::SLOT *
           sizeof(float);
  if (CC == 32 && CF == 16)
    return (size_t)tw_chunks(tw_geo<32, 16>(B, in, nullptr, out)) * TwTile<32, 16>::KP * TwTile<32, 16>::SLOT *
           sizeof(float);
  return 0;
}

void launch_conv3d_t2_wgrad(const float* x, const float* gy, int B, int CC, int CF, const int* in, const int* crop,
                            const int* out, float* part, float* dw, hipStream_t s) {
  if (CC == 64 && CF == 32) tw_launch<64, 32>(x, gy, B, in, crop, out, part, dw, s);
  else if (CC == 32 && CF == 16) tw_launch<32, 16>(x, gy, B, in, crop, out, part, dw, s);
}

}  // namespace mvs
