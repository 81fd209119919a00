// deconv3d_region_bwd.hip -- backward of the regulariser's last transposed region convolution under autograd
// (deconv_1_0, 16 -> 8, model.py:87: ConvTranspose3d(3, stride 2) from the M-region tensor to the whole volume;
// mvs_amd/region_train.py _D1Box; the forward is deconv3d_region.hip in raw mode).  With o = 2 i + t - crop per
// dim, t = 0..2, and gy the output gradient on the box [0, out):
//
//   gx[b][ci][i]  = sum over co and t of gy[b][co][2 i + t - crop] * W[ci][co][t]
//   dW[ci][co][t] = sum over the batch and every input voxel i of x[b][ci][i] * gy[b][co][2 i + t - crop]
//
// (terms whose gy index is off the box are absent).  gy is NCDHW [B][8][Oz][Oy][Ox], the layout autograd delivers
// it in behind the NCDHW forward, read in place; x and gx are NCDHW [B][16][I...] or channels-last [B][I...][16]
// (XCL), gx in x's layout.  Products and sums are fp32; sample and row addresses are 64-bit (gy passes 2^32
// bytes at the training shapes).
//
// Input gradient: a gather, one thread per input voxel and its 16 channels, no atomics.  Per tap plane tz the
// thread reads the plane's 3 x 3 x 8 values of gy and runs 16 chains of 72 fmaf (ty, tx, co in that order) with
// the weights as workgroup-uniform scalar loads (deconv3d_region.hip's scheme); the three planes' sums are added
// once as (p0 + p1) + p2.
//
// Weight gradient: wgrad_taprow.h's plan with K = the coarse voxels, a tile kDwTR coarse rows (flattened b, iz,
// iy).  Wave kp runs the rows kp, kp + 4, ... of each tile (four partial sums of K, a slot each).  Per K-step of
// four coarse voxels a wave issues two v_mfma_f32_16x16x4_f32: M = the 16 ci, N = 8 co x the taps (tx 0 | tx 1),
// then N = 8 co x (tx 2 | unused).  Per tile the workgroup stages
//   x:  channels-last: 16 voxel records of 16 floats per row (A read: lane (m, kq) at kq * 16 + m, 64 consecutive
//       floats); NCDHW: 16 channel records of 18 floats per row (lane at m * 18 + kq: the 32 lanes of a half on
//       32 banks);
//   gy: the tap row's fine row (b, 2 iz - cz + tz, 2 iy - cy + ty) of each coarse row, per co the 34 fine voxels
//       2 x0 - cx + j as a record of 36 floats (B read: lane (co, h, kq) at co * 36 + 2 kq + h: 32 banks per half).
// Coarse rows whose fine row is off the box are skipped (their products are all 0).  The slot is [27][16][8]; a
// tap's entries come from one of the nine tap rows' workgroups.
#include "launchers.h"
#include "wgrad_taprow.h"

namespace mvs {
namespace {

constexpr int kDCin = 16, kDCout = 8;

// ---------------------------------------------------------------------------------------------------------
// input gradient
// ---------------------------------------------------------------------------------------------------------
struct DgGeo {
  int Iz, Iy, Ix;
  int Oz, Oy, Ox;
  int cz, cy, cx;
  unsigned total;   // B * Iz * Iy * Ix input voxels
};

template <bool XCL>
__global__ __launch_bounds__(kBlock) void deconv3d_dgrad_kernel(const float* __restrict__ gy,
                                                               const float* __restrict__ w27,
                                                               float* __restrict__ gx, DgGeo g) {
  const size_t gid = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (gid >= g.total) return;
  const int ix = (int)(gid % g.Ix);
  size_t t = gid / g.Ix;
  const int iy = (int)(t % g.Iy);
  t /= g.Iy;
  const int iz = (int)(t % g.Iz);
  const int b = (int)(t / g.Iz);
  const size_t plane = (size_t)g.Oz * g.Oy * g.Ox, ivol = (size_t)g.Iz * g.Iy * g.Ix;
  const float* gyb = gy + (size_t)b * kDCout * plane;
  const const_float* wc = (const const_float*)uniform_ptr(w27);   // [27][ci][co]: scalar loads
  const int ox0 = 2 * ix - g.cx, oy0 = 2 * iy - g.cy, oz0 = 2 * iz - g.cz;
  bool okx[3];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx) okx[tx] = ox0 + tx >= 0 && ox0 + tx < g.Ox;

  float s[kDCin];
#pragma unroll
  for (int ci = 0; ci < kDCin; ++ci) s[ci] = 0.0f;
#pragma unroll 1
  for (int tz = 0; tz < 3; ++tz) {
    float p[kDCin];
#pragma unroll
    for (int ci = 0; ci < kDCin; ++ci) p[ci] = 0.0f;
    const int oz = oz0 + tz;
    const bool okz = oz >= 0 && oz < g.Oz;
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      const int oy = oy0 + ty;
      const bool okzy = okz && oy >= 0 && oy < g.Oy;
      const size_t row = okzy ? ((size_t)oz * g.Oy + oy) * g.Ox : 0;
      float v[3][kDCout];
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int co = 0; co < kDCout; ++co)
          v[tx][co] = (okzy && okx[tx]) ? gyb[(size_t)co * plane + row + (size_t)(ox0 + tx)] : 0.0f;
      asm volatile("" ::: "memory");   // one tap row of weights in SGPRs at a time
      const const_float* wr = wc + (size_t)((tz * 3 + ty) * 3) * (kDCin * kDCout);
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int co = 0; co < kDCout; ++co)
#pragma unroll
          for (int ci = 0; ci < kDCin; ++ci)
            p[ci] = fmaf(v[tx][co], wr[(tx * kDCin + ci) * kDCout + co], p[ci]);
    }
    // (p0 + p1) + p2
#pragma unroll
    for (int ci = 0; ci < kDCin; ++ci) s[ci] += p[ci];
  }
  if constexpr (XCL) {
    float* o = gx + gid * kDCin;
#pragma unroll
    for (int q = 0; q < kDCin / 4; ++q)
      *reinterpret_cast<f4v*>(o + 4 * q) = f4v{s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]};
  } else {
    float* o = gx + (size_t)b * kDCin * ivol + ((size_t)iz * g.Iy + iy) * g.Ix + ix;
#pragma unroll
    for (int ci = 0; ci < kDCin; ++ci) o[(size_t)ci * ivol] = s[ci];
  }
}

// ---------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------
constexpr int kDwTX = kTapRowTX;         // coarse x-voxels of a tile
constexpr int kDwTR = 16;                // coarse rows of a tile
constexpr int kDwKP = 4;                 // partial sums of K per workgroup: the waves split the tile's rows
constexpr int kDwFX = 2 * kDwTX + 2;     // staged fine voxels per (row, co)
constexpr int kDwFS = 36;                // floats per staged gy record
constexpr int kDwXS = 18;                // floats per staged x channel record (NCDHW)
constexpr int kDwXRow = kDwXS * kDCin;   // floats per staged x row (either layout: 256 used channels-last)
constexpr int kDwSlot = 27 * kDCin * kDCout;
static_assert(kDwFS % 32 == 4 && kDwFS >= kDwFX, "B reads: co * FS + 2 kq + h over 32 banks per half");
static_assert(kDwXS % 32 == 18 && kDwXS >= kDwTX, "A reads (NCDHW): m * XS + kq over 32 banks per half");
static_assert(kDwTR % kDwKP == 0 && kBlock == 64 * kDwKP, "one wave per K part");

struct DwGeo {
  int B;
  int Iz, Iy, Ix;
  int Oz, Oy, Ox;
  int cz, cy, cx;
  TapRowGeo t;           // rows: B * Iz * Iy coarse rows
};

template <bool XCL>
__global__ __launch_bounds__(kBlock) void deconv3d_wgrad_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ gy,
                                                               float* __restrict__ part, DwGeo g) {
  __shared__ __attribute__((aligned(16))) float cs[kDwTR * kDwXRow];
  __shared__ __attribute__((aligned(16))) float fs[kDwTR * kDCout * kDwFS];
  const int tid = (int)threadIdx.x, lane = tid & 63, kp = tid >> 6;
  const int m = lane & 15, kq = lane >> 4;
  const TapRowBlock blk = taprow_block();
  const size_t plane = (size_t)g.Oz * g.Oy * g.Ox, ivol = (size_t)g.Iz * g.Iy * g.Ix;
  // A: lane (m, kq) supplies x[voxel 4 s + kq][ci = m]; B: lane (n = m, kq) supplies gy[co = n & 7][fine voxel
  // 2 (4 s + kq) + tx], tx = n >> 3 (first MFMA) or 2 (second; its columns 8-15 are not stored)
  const int aoff = XCL ? kq * kDCin + m : m * kDwXS + kq, astep = XCL ? 4 * kDCin : 4;
  const int boff0 = (m & 7) * kDwFS + 2 * kq + (m >> 3), boff1 = (m & 7) * kDwFS + 2 * kq + 2;

  f4v acc[2];
  acc[0] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
  acc[1] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  taprow_walk<kDwTR>(
      blk, g.t,
      [&](int R, long long& oc, long long& of) {
        const int iy = R % g.Iy, t = R / g.Iy;
        const int iz = t % g.Iz, b = t / g.Iz;
        const int fz = 2 * iz - g.cz + blk.tz, fy = 2 * iy - g.cy + blk.ty;
        // x[b][iz][iy][0][0] (channels-last) or x[b][0][iz][iy][0] (NCDHW)
        oc = XCL ? (long long)R * g.Ix * kDCin
                 : (long long)b * kDCin * (long long)ivol + ((long long)iz * g.Iy + iy) * g.Ix;
        if (fz >= 0 && fz < g.Oz && fy >= 0 && fy < g.Oy)
          of = (long long)b * kDCout * (long long)plane + ((long long)fz * g.Oy + fy) * g.Ox;   // gy[b][0][fz][fy][0]
      },
      [&](int x0, const long long* rowc, const long long* rowf) {
        const int fx0 = 2 * x0 - g.cx;   // the tile's first fine voxel along x (may be negative)
        // stage x; voxels past the extent read 0 (their products vanish)
        if constexpr (XCL) {   // items (row, voxel, 16-byte chunk), chunk fastest: coalesced channels-last loads
          for (int e = tid; e < kDwTR * kDwTX * (kDCin / 4); e += kBlock) {
            const int c4 = e % (kDCin / 4), v = e / (kDCin / 4);
            const int r = v / kDwTX, xi = v % kDwTX;
            if (rowf[r] < 0) continue;
            f4v val{0.0f, 0.0f, 0.0f, 0.0f};
            if (x0 + xi < g.Ix)
              val = *reinterpret_cast<const f4v*>(x + rowc[r] + (long long)(x0 + xi) * kDCin + 4 * c4);
            *reinterpret_cast<f4v*>(cs + r * kDwXRow + xi * kDCin + 4 * c4) = val;
          }
        } else {               // items (row, channel, voxel), voxel fastest
          for (int e = tid; e < kDwTR * kDCin * kDwTX; e += kBlock) {
            const int xi = e % kDwTX, t = e / kDwTX;
            const int ci = t % kDCin, r = t / kDCin;
            if (rowf[r] < 0) continue;
            float val = 0.0f;
            if (x0 + xi < g.Ix) val = x[rowc[r] + (long long)ci * (long long)ivol + (x0 + xi)];
            cs[r * kDwXRow + ci * kDwXS + xi] = val;
          }
        }
        // stage gy: items (row, co, fine voxel j), j fastest; voxels off the row read 0
        for (int e = tid; e < kDwTR * kDCout * kDwFX; e += kBlock) {
          const int j = e % kDwFX, t = e / kDwFX;
          const int co = t % kDCout, r = t / kDCout;
          const long long o = rowf[r];
          if (o < 0) continue;
          const int fx = fx0 + j;
          float val = 0.0f;
          if (fx >= 0 && fx < g.Ox) val = gy[o + (long long)co * (long long)plane + fx];
          fs[(r * kDCout + co) * kDwFS + j] = val;
        }
        __syncthreads();
        // the K-steps of the staged tile
#pragma unroll 1
        for (int r = kp; r < kDwTR; r += kDwKP) {
          if (rowf[r] < 0) continue;   // wave-uniform: no such row, or its fine row is off the box
          const float* ar = cs + r * kDwXRow + aoff;
          const float* br = fs + r * kDCout * kDwFS;
#pragma unroll
          for (int s = 0; s < kDwTX / 4; ++s) {
            const float a = ar[s * astep];
            const float b0 = br[boff0 + 8 * s], b1 = br[boff1 + 8 * s];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1], 0, 0, 0);
          }
        }
      });
  // partial slot [27][ci][co]: acc[q][i] = D[ci = 4 kq + i][n = m]: tap tx = n >> 3 (q = 0) or 2 (q = 1, n < 8)
  float* slot = part + ((size_t)blk.chunk * kDwKP + kp) * kDwSlot;
  const int co = m & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    slot[((blk.row_tap * 3 + (m >> 3)) * kDCin + 4 * kq + i) * kDCout + co] = acc[0][i];
    if (m < 8) slot[((blk.row_tap * 3 + 2) * kDCin + 4 * kq + i) * kDCout + co] = acc[1][i];
  }
}

DwGeo dw_geo(int B, const int* in, const int* crop, const int* out) {
  DwGeo g;
  g.B = B;
  g.Iz = in[0], g.Iy = in[1], g.Ix = in[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.cz = crop ? crop[0] : 0, g.cy = crop ? crop[1] : 0, g.cx = crop ? crop[2] : 0;
  g.t = taprow_geo(B * g.Iz * g.Iy, g.Ix, kDwTR);
  return g;
}

}  // namespace

size_t deconv3d_wgrad_workspace_bytes(int B, const int* in, const int* out) {
  return taprow_workspace_bytes(dw_geo(B, in, nullptr, out).t, kDwKP, kDwSlot);
}

void launch_deconv3d_wgrad(const float* x, bool x_cl, const float* gy, int B, const int* in, const int* crop,
                           const int* out, float* part, float* dw, hipStream_t s) {
  const DwGeo g = dw_geo(B, in, crop, out);
  if (x_cl)
    hipLaunchKernelGGL((deconv3d_wgrad_kernel<true>), taprow_grid(g.t), dim3(kBlock), 0, s, x, gy, part, g);
  else
    hipLaunchKernelGGL((deconv3d_wgrad_kernel<false>), taprow_grid(g.t), dim3(kBlock), 0, s, x, gy, part, g);
  launch_wgrad_reduce(part, taprow_chunks(g.t) * kDwKP, kDCin, kDCout, dw, s);
}

void launch_deconv3d_dgrad(const float* gy, const float* w27, float* gx, bool x_cl, int B, const int* in,
                           const int* crop, const int* out, hipStream_t s) {
  DgGeo g;
  g.Iz = in[0], g.Iy = in[1], g.Ix = in[2];
  g.Oz = out[0], g.Oy = out[1], g.Ox = out[2];
  g.cz = crop[0], g.cy = crop[1], g.cx = crop[2];
  g.total = (unsigned)B * (unsigned)in[0] * (unsigned)in[1] * (unsigned)in[2];
  const dim3 grid((g.total + kBlock - 1) / kBlock);
  if (x_cl) hipLaunchKernelGGL((deconv3d_dgrad_kernel<true>), grid, dim3(kBlock), 0, s, gy, w27, gx, g);
  else hipLaunchKernelGGL((deconv3d_dgrad_kernel<false>), grid, dim3(kBlock), 0, s, gy, w27, gx, g);
}

}  // namespace mvs
