// conv3d_region.hip -- the regulariser's region convolutions (CostVolumeReg, regulariser.py; the
// reference's model.py:76-121) as implicit GEMMs on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact
// fp32, one rounding per product, the f32 VALU's peak rate without its operand traffic), with the
// eval-mode BatchNorm + ReLU that follows every one of them fused into the epilogue.
//
// forward_live evaluates the U-Net level k only on its live region.  The region
// tensors live channels-last, x[b][z][y][x][c] (NDHWC, the GEMM's K = channel axis contiguous),
// with their box origin (o0) in the volume; three forms:
//   S1  conv_k_1:     3x3x3, stride 1, padding 1 (zero outside the VOLUME), region -> region
//   S2  conv_k_0:     3x3x3, stride 2, padding P (config.py:20), the full cost volume (NCDHW, or
//                     the fused kernel's channel-quad NC4DHW4: 4 channels per 16-byte load) ->
//                     region: output o reads inputs 2 o - P + t, t = 0..2, per dim
//   T2  deconv_k_0:   ConvTranspose3d 3x3x3, stride 2, padding P, region -> region: output o
//                     gathers inputs i = (o + P - t) / 2 for t of o + P's parity (1 or 2 taps per
//                     dim); outputs are processed by parity class (8 launches' worth of grid.y), so
//                     every voxel of a 16-voxel MFMA row block has the same taps; the input may be
//                     the sum of two region tensors (model.py:119-121's `y3 + y2`, `y2 + y1`).  That is
//                     the class kernel (MVS_CONV_PER_LANE, the stacked input gradient); the forward's
//                     default for 32 -> 16 is conv3d_t2_cells_kernel below, one pass per input cell,
//                     bit-equal.
// GEMM per sample: rows = output voxels of the region (flattened z, y, x; parity class for T2),
// columns = output channels, K = (tap, input channel).  A wave owns 2 x 16 rows and every column
// block (CO / 16); per (tap, 16-channel block) each lane loads 4 consecutive channels of its row's
// input voxel (channels-last: one 16-byte load; S2 reads the NCDHW volume per channel) and of its
// column's weights, which feed 4 MFMAs (K-step s takes component s).  Weights arrive as
// w[tap][co][ci] (ops.py transposes nn.Conv3d / nn.ConvTranspose3d's layouts).  Products are summed
// per tap over channels in a fixed order -- MIOpen's kernels sum in other orders; same products,
// fp32 rounding-level differences.
#include "launchers.h"
#include "region_conv.h"

#include <type_traits>
#include <utility>

namespace mvs {
namespace {

// (output voxels per wave: RB MFMA row blocks of 16 -- template; 2 by default)
struct Geo {
  int n[3];     // volume dims (D, H, W)
  int o0[3];    // output region origin
  int on[3];    // output region size
  int i0[3];    // input region origin (S1, T2; S2: the box of the volume the input tensor holds)
  int in[3];    // input region size (S1, T2; S2: the box size, = n when the whole volume is given)
  int pad[3];   // P (S2, T2)
  int out_cf;   // 1: output region tensor channels-first y[b][co][z][y][x] (else channels-last)
  int in_c4;    // S2: the volume is channel-quad x[b][C/4][D][H][W][4], fp32 (1), bf16 (2) or the split
                //     cost volume (3, split.h: fp32 re-formed on load as (hi + lo) 2^-e); 0 NCDHW
  const uint32_t* absmax;   // in_c4 = 3: the volume's bound words (its scale)
  uint32_t* y_bound;        // optional: the output's bound words (split.h), raised in the epilogue
  int st0[3];   // the output region's place in the stored tensor: y holds a box of size stn whose
  int stn[3];   //   voxel st0 is the region's first (default 0 / on: y is the region)
};

__device__ inline void store_out(float* __restrict__ y, const Geo& g, int b, int co, int vz, int vy, int vx,
                                 int CO, float v) {
  const size_t vox = ((size_t)(vz + g.st0[0]) * g.stn[1] + (vy + g.st0[1])) * g.stn[2] + (vx + g.st0[2]);
  const size_t rvol = (size_t)g.stn[0] * g.stn[1] * g.stn[2];
  if (g.out_cf) y[((size_t)b * CO + co) * rvol + vox] = v;
  else y[((size_t)b * rvol + vox) * CO + co] = v;
}

// QM (S2 only): input layout of the volume -- 0 NCDHW, 1 fp32 channel quads, 2 bf16 channel quads --
// 4 channels-last x[b][z][y][x][c] (the transposed layers' input gradient: gy as the volume) --
// a template parameter, so the K loop has no per-load layout branches and (S1 / S2: no parity
// classes) unrolls into one basic block the scheduler can software-pipeline (loads of later taps
// issued under the MFMAs of earlier ones)
// CLS (T2 only): the parity class (pz, py, px) = bits (2, 1, 0) as a COMPILE-TIME constant, so the tap
// loops unroll to exactly the class's 1-8 taps in one basic block (the loads of every tap issued ahead of
// the MFMAs); the kernel below dispatches on blockIdx.y.  -1 (S1 / S2): no classes.
// PS: independent partial sums per output.  1: one accumulation chain over every (tap, channel) -- every
// forward instantiation.  4 (CI = 112, the stacked stride-2 layers' input gradient): one chain per channel
// group (16 | 32 | 32 | 32: conv_1_0, conv_2_0 and the halves of conv_3_0), added once in the epilogue as
// (p0 + p1) + (p2 + p3) -- a chain is at most 8 taps x 32 channels long instead of 8 x 112.  3 (S2 from the
// channels-last volume, the transposed layers' input gradient): one chain per tap plane tz, added once as
// (p0 + p1) + p2 -- a chain is 9 taps x CI channels long instead of 27 x CI.
template <int MODE, int CI, int CO, int RB, int QM, int CLS, int PS = 1>
__device__ __forceinline__ void region_conv(
    const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ w,
    float* __restrict__ y, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift,
    const float* __restrict__ bn_mean, const Geo& g) {
  constexpr int NB = CO / 16;          // column blocks
  static_assert(CI % 16 == 0 && CO % 16 == 0, "channel counts in multiples of 16");
  static_assert((MODE == kT2) == (CLS >= 0), "parity classes: transposed convolutions");
  static_assert(PS == 1 || (PS == 4 && CI == 112) || (PS == 3 && MODE == kS2 && QM == 4),
                "partial sums: the input gradients only");
  static_assert(QM != 4 || MODE == kS2, "channels-last volume: the stride-2 mode");
  constexpr bool kPlanes = MODE == kS2 && QM != 4;   // the input is read per channel plane / quad plane
  const int lane = (int)threadIdx.x & 63;
  const int m = lane & 15, kq = lane >> 4;   // MFMA row / K index of this lane's A value
  const int b = (int)blockIdx.z;

  // ---- rows of this wave: parity class (T2) or the whole region ----
  int cf[3], cn[3];
  constexpr int par[3] = {CLS >= 0 ? (CLS >> 2) & 1 : 0, CLS >= 0 ? (CLS >> 1) & 1 : 0, CLS >= 0 ? CLS & 1 : 0};
  if constexpr (MODE == kT2) {
#pragma unroll
    for (int d = 0; d < 3; ++d) class_dim(g.o0[d], g.on[d], g.pad[d], par[d], cf[d], cn[d]);
  } else {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      cf[d] = g.o0[d];
      cn[d] = g.on[d];
    }
  }
  const int rows = cn[0] * cn[1] * cn[2];
  const int sx = QM == 3 ? cv_split_exponent(g.absmax) : 0;
  const int step = MODE == kT2 ? 2 : 1;
  constexpr int kRows = 16 * RB;
  // XCD-contiguous row blocks (gridDim.x is a multiple of 8): workgroups are dealt round-robin over
  // the 8 XCDs, so without the remap the neighbours that share input rows / planes (the next output
  // row, the next plane ~ one row of workgroups later) sit in 8 different L2s; remapped, each XCD
  // sweeps a contiguous run of the region and re-reads them from its own L2
  const int bx = xcd_work_id((int)blockIdx.x, (int)gridDim.x);
  const int row0 = (bx * (kBlock / 64) + ((int)threadIdx.x >> 6)) * kRows;
  if (row0 >= rows) return;   // wave-uniform; no barriers in this kernel

  // per row block: this lane's input base voxel in the addressed space (the volume for S2, the
  // input region for S1 / T2) and, per dim and tap, whether the tap's input exists; input voxel of
  // tap t = base + delta(t) per dim with delta = t (S1, S2) or -(t >> 1) (T2, taps of the class's
  // parity: t = par, par + 2)
  int lim[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) lim[d] = g.in[d];
  int lin[RB];            // linear index of the base voxel (may be negative; masked)
  unsigned vm[RB][3];     // per dim: bit t = tap t's input exists
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int r = row0 + rb * 16 + m;
    const bool ok = r < rows;
    const int rr = ok ? r : 0;
    const int jx = rr % cn[2], t = rr / cn[2];
    const int jy = t % cn[1], jz = t / cn[1];
    const int o[3] = {cf[0] + step * jz, cf[1] + step * jy, cf[2] + step * jx};
    int bs[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if constexpr (MODE == kS1) bs[d] = o[d] - 1 - g.i0[d];
      else if constexpr (MODE == kS2) bs[d] = 2 * o[d] - g.pad[d] - g.i0[d];   // taps off the box: off the volume
      else bs[d] = ((o[d] + g.pad[d] - par[d]) >> 1) - g.i0[d];
      unsigned mk = 0;
#pragma unroll
      for (int tt = 0; tt < 3; ++tt) {
        const int dl = MODE == kT2 ? -(tt >> 1) : tt;
        const bool in = ok && bs[d] + dl >= 0 && bs[d] + dl < lim[d] && !(MODE == kT2 && ((tt & 1) != par[d]));
        mk |= in ? (1u << tt) : 0u;
      }
      vm[rb][d] = mk;
    }
    lin[rb] = (bs[0] * lim[1] + bs[1]) * lim[2] + bs[2];
  }

  f4v acc[PS][RB][NB];
#pragma unroll
  for (int ps = 0; ps < PS; ++ps)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[ps][rb][nb] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  // buffer descriptors (workgroup-uniform bases; out-of-range offsets read 0): S2 the sample's
  // volume (channel-quad: quads cb*4 .. cb*4+3 per channel block; NCDHW: 16 channel planes per
  // block), S1 / T2 the sample's region tensor (and addend)
  const size_t rvol = (size_t)g.in[0] * g.in[1] * g.in[2];
  // (S2: rvol = voxels of the (boxed) volume per channel plane / quad plane)
  const int sy = lim[2], sz = lim[1] * lim[2];
  // ---- K loop: taps by rows (tz, ty); per row and 16-channel block the A values of its (up to)
  // three x taps and every row block and the matching weights are loaded together, then fed to
  // the MFMAs (3x the loads in flight of a tap-at-a-time loop) ----
#pragma unroll
  for (int tz = 0; tz < 3; ++tz) {
    if (MODE == kT2 && ((tz & 1) != par[0])) continue;   // t of o + P's parity only
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      if (MODE == kT2 && ((ty & 1) != par[1])) continue;
      const int dz = MODE == kT2 ? -(tz >> 1) : tz, dy = MODE == kT2 ? -(ty >> 1) : ty;
      // input voxel of this lane's row per (x tap, row block); kOob = no input (reads 0)
      uint32_t vox[3][RB];
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const int dx = MODE == kT2 ? -(tx >> 1) : tx;
          const bool ok = ((vm[rb][0] >> tz) & (vm[rb][1] >> ty) & (vm[rb][2] >> tx) & 1u) != 0;
          vox[tx][rb] = ok ? (uint32_t)(lin[rb] + dz * sz + dy * sy + dx) : kOob;
        }
      // K = each tap's CI channels in blocks of 16: in K-step s of block cb, lane (m, kq) supplies
      // channel cb * 16 + 4 kq + s -- one 16-byte load per lane (4 consecutive channels of its row's
      // voxel, channels-last; of its column's weight row, w[tap][co][ci]) feeds 4 MFMAs
#pragma unroll
      for (int cb = 0; cb < CI / 16; ++cb) {
        const int c4 = cb * 16 + kq * 4;
        const int ps = PS == 1 ? 0 : PS == 3 ? tz : (cb + 1) / 2;   // this (tap plane's /) channel block's partial sum
        Rsrc rs, rs2;
        if constexpr (kPlanes) {
          if constexpr (QM == 2)   // bf16 quads: 8 bytes per voxel and quad
            rs = make_rsrc(reinterpret_cast<const char*>(x) + ((size_t)b * (CI / 4) + cb * 4) * rvol * 8,
                           (uint32_t)(rvol * 32));
          else if constexpr (QM == 1 || QM == 3)
            rs = make_rsrc(x + ((size_t)b * (CI / 4) + cb * 4) * rvol * 4, (uint32_t)(rvol * 64));
          else
            rs = make_rsrc(x + ((size_t)b * CI + cb * 16) * rvol, (uint32_t)(rvol * 64));
        } else {
          rs = make_rsrc(x + (size_t)b * rvol * CI, (uint32_t)(rvol * CI * 4));
          if (x2) rs2 = make_rsrc(x2 + (size_t)b * rvol * CI, (uint32_t)(rvol * CI * 4));
        }
        f4v a[3][RB], bw[3][NB];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          if (MODE == kT2 && ((tx & 1) != par[2])) continue;
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            const uint32_t vx = vox[tx][rb];
            f4v v;
            if constexpr (kPlanes) {
              if constexpr (QM == 2) {   // the bf16 quad: one 8-byte load, widened (exact)
                typedef __attribute__((ext_vector_type(2))) unsigned v2u;
                const v2u p = __builtin_amdgcn_raw_buffer_load_b64(
                    rs, (int)(vx == kOob ? kOob : ((uint32_t)kq * (uint32_t)rvol + vx) * 8u), 0, 0);
                v = f4v{__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xFFFF0000u),
                          __uint_as_float(p.y << 16), __uint_as_float(p.y & 0xFFFF0000u)};
              } else if constexpr (QM == 3) {   // split quad: 16-byte load, (hi + lo) 2^-sx (exact sum)
                v = unsplit4(__builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                 rs, (int)(vx == kOob ? kOob : ((uint32_t)kq * (uint32_t)rvol + vx) * 16u), 0, 0)),
                             sx);
              } else if constexpr (QM == 1) {   // the quad (c4 / 4) of the voxel: one 16-byte load
                v = ld4(rs, vx == kOob ? kOob : ((uint32_t)kq * (uint32_t)rvol + vx) * 16u, 0);
              } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                  v[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                      rs, (int)(vx == kOob ? kOob : ((uint32_t)(kq * 4 + q) * (uint32_t)rvol + vx) * 4u), 0, 0));
              }
            } else {
              const uint32_t eo = vx == kOob ? kOob : (vx * (uint32_t)CI + (uint32_t)c4) * 4u;
              v = ld4(rs, eo, 0);
              if (x2) v += ld4(rs2, eo, 0);
            }
            a[tx][rb] = v;
          }
          const float* wt = w + (size_t)((tz * 3 + ty) * 3 + tx) * CO * CI;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            bw[tx][nb] = *reinterpret_cast<const f4v*>(wt + (size_t)(nb * 16 + m) * CI + c4);
        }
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
          if (MODE == kT2 && ((tx & 1) != par[2])) continue;
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
              for (int nb = 0; nb < NB; ++nb)
                acc[ps][rb][nb] =
                    __builtin_amdgcn_mfma_f32_16x16x4f32(a[tx][rb][s], bw[tx][nb][s], acc[ps][rb][nb], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: eval BN + ReLU, NDHWC store.  acc[rb][nb][r] = (row (lane>>4)*4 + r, col lane&15)
  float vmax = 0.0f;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = nb * 16 + m;
    const float sc = bn_scale ? bn_scale[co] : 1.0f, sh = bn_scale ? bn_shift[co] : 0.0f,
                mu = bn_scale ? bn_mean[co] : 0.0f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rb * 16 + kq * 4 + r;
        if (row >= rows) continue;
        const int jx = row % cn[2], t = row / cn[2];
        const int jy = t % cn[1], jz = t / cn[1];
        const int vz = cf[0] + step * jz - g.o0[0], vy = cf[1] + step * jy - g.o0[1],
                  vx = cf[2] + step * jx - g.o0[2];
        float v = acc[0][rb][nb][r];
        if constexpr (PS == 4)
          v = (v + acc[1][rb][nb][r]) + (acc[PS - 2][rb][nb][r] + acc[PS - 1][rb][nb][r]);
        if constexpr (PS == 3) v = (v + acc[1][rb][nb][r]) + acc[PS - 1][rb][nb][r];
        if (bn_scale) v = fmaxf((v - mu) * sc + sh, 0.0f);
        vmax = fmaxf(vmax, fabsf(v));
        store_out(y, g, b, co, vz, vy, vx, CO, v);
      }
  }
  if (g.y_bound) bound_update(g.y_bound, vmax);
}

template <int MODE, int CI, int CO, int RB, int QM = 0, int PS = 1>
__global__ __launch_bounds__(kBlock) void conv3d_region_kernel(
    const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ w,
    float* __restrict__ y, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift,
    const float* __restrict__ bn_mean, Geo g) {
  if constexpr (MODE == kT2) {
    switch (blockIdx.y) {   // workgroup-uniform
#define MVS_T2_CLASS(c) \
  case c: region_conv<MODE, CI, CO, RB, QM, c, PS>(x, x2, w, y, bn_scale, bn_shift, bn_mean, g); break;
      MVS_T2_CLASS(0) MVS_T2_CLASS(1) MVS_T2_CLASS(2) MVS_T2_CLASS(3)
      MVS_T2_CLASS(4) MVS_T2_CLASS(5) MVS_T2_CLASS(6) MVS_T2_CLASS(7)
#undef MVS_T2_CLASS
      default: break;
    }
  } else {
    region_conv<MODE, CI, CO, RB, QM, -1, PS>(x, x2, w, y, bn_scale, bn_shift, bn_mean, g);
  }
}

template <int MODE, int CI, int CO, int RB, int QM = 0, int PS = 1>
void launch_mode(const float* x, const float* x2, const float* w, float* y, const float* sc, const float* sh,
                 const float* mu, int B, const Geo& g, hipStream_t s) {
  hipLaunchKernelGGL((conv3d_region_kernel<MODE, CI, CO, RB, QM, PS>), region_grid(MODE, RB, B, g.on), dim3(kBlock), 0, s,
                     x, x2, w, y, sc, sh, mu, g);
}

// ---- transposed convolutions, one register-tiled pass per input cell (deconv_2_0) ----
// The class kernel above walks the output eight times, once per parity class, and every class fetches its
// own taps' input voxels: over the classes each voxel's 16-channel block is loaded 27 times (54 with the
// addend), and within a class consecutive rows are outputs two apart in x (4-byte stores with gaps the other
// x parity fills from another workgroup).  Here a GEMM row is a CELL c = (o + P) >> 1 per dim: its 2 x 2 x 2
// outputs 2 c - P + par read only the 2 x 2 x 2 inputs {c, c - 1}^3 (tap t = par + 2 j reads c - j), so the
// lane loads each of them once and feeds all eight classes' accumulators from registers -- no LDS, no
// barriers.  A wave owns RB row blocks of 16 consecutive cells along x (row blocks of every (cell-z, cell-y)
// line, flattened); lane (m, kq) supplies channels cb * 16 + 4 kq + s of row m as in the class kernel.
// Order: the tap rows (tz, ty) are visited by the input row (jz, jy) = (tz >> 1, ty >> 1) they read --
// (0,0) (0,1) (1,0) (1,1) | (0,2) (1,2) | (2,0) (2,1) | (2,2) -- so only one input row (2 voxels x CI
// channels per row block) is live at a time; within every class that is still ascending (tz, ty), then
// channel block, then tx, then K-step: each accumulator sees the class kernel's products in the class
// kernel's order, and every output is bit-equal to region_conv<kT2, ..., CLS>.  The eight classes' chains
// are independent, which hides the dependent-MFMA latency the 1-tap class cannot hide on its own.
// Epilogue (eval BN + ReLU; no bound words): lane (m, kq) holds, per channel and (pz, py), the 2 x 4 outputs of cells 4 kq .. 4 kq + 3: 8
// consecutive x.  Channels-first they go out as 16-byte / 8-byte vectors on the address's alignment (single
// dwords only at the two ends of a lane's run when it starts on an odd element, and at the region's edges);
// channels-last as 16 lanes x 4 B per voxel, as the class kernel.
typedef float f2v __attribute__((ext_vector_type(2)));

// v[0 .. 8) to p[0 .. 8), elements lo <= i < hi only; A = (element index of p) mod 4
template <int A>
__device__ __forceinline__ void store_run8(float* __restrict__ p, const float (&v)[8], int lo, int hi) {
  auto st1 = [&](int i) {
    if (i >= lo && i < hi) p[i] = v[i];
  };
  auto st2 = [&](int i) {
    if (i >= lo && i + 2 <= hi) *reinterpret_cast<f2v*>(p + i) = f2v{v[i], v[i + 1]};
    else st1(i), st1(i + 1);
  };
  auto st4 = [&](int i) {
    if (i >= lo && i + 4 <= hi) *reinterpret_cast<f4v*>(p + i) = f4v{v[i], v[i + 1], v[i + 2], v[i + 3]};
    else st2(i), st2(i + 2);
  };
  if constexpr (A == 0) st4(0), st4(4);
  else if constexpr (A == 2) st2(0), st4(2), st2(6);
  else if constexpr (A == 1) st1(0), st2(1), st4(3), st1(7);
  else st1(0), st4(1), st2(5), st1(7);
}

template <int CI, int CO, int RB, bool X2>
__global__ __launch_bounds__(kBlock) void conv3d_t2_cells_kernel(
    const float* __restrict__ x, const float* __restrict__ x2, const float* __restrict__ w,
    float* __restrict__ y, const float* __restrict__ bn_scale, const float* __restrict__ bn_shift,
    const float* __restrict__ bn_mean, Geo g) {
  constexpr int NB = CO / 16, CB = CI / 16;
  static_assert(CI % 16 == 0 && CO % 16 == 0, "channel counts in multiples of 16");
  const int lane = (int)threadIdx.x & 63;
  const int m = lane & 15, kq = lane >> 4;
  const int b = (int)blockIdx.z;

  // ---- cells: per dim every cell with an output in the region; row blocks of 16 cells along x ----
  int cf[3], cn[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) cell_dim(g.o0[d], g.on[d], g.pad[d], cf[d], cn[d]);
  const int nbx = (cn[2] + 15) >> 4;
  const int blocks = cn[0] * cn[1] * nbx;
  const int bx = xcd_work_id((int)blockIdx.x, (int)gridDim.x);
  const int blk0 = uniform((bx * (kBlock / 64) + ((int)threadIdx.x >> 6)) * RB);
  if (blk0 >= blocks) return;   // wave-uniform; no barriers in this kernel

  // per row block (wave-uniform): its line and first cell; per lane: the linear index of cell m's input
  // voxel c in the input region and, per dim, whether inputs c (bit 0) and c - 1 (bit 1) exist
  const int sy = g.in[2], sz = g.in[1] * g.in[2];
  bool live[RB];
  int lz[RB], ly[RB], xb[RB], lin[RB];
  unsigned vm[RB][3];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    live[rb] = blk0 + rb < blocks;
    const int blk = live[rb] ? blk0 + rb : 0;
    xb[rb] = blk % nbx;
    const int line = blk / nbx;
    ly[rb] = line % cn[1];
    lz[rb] = line / cn[1];
    const int ci[3] = {lz[rb], ly[rb], xb[rb] * 16 + m};   // cell index in the cell box
    int bs[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      bs[d] = cf[d] + ci[d] - g.i0[d];
      unsigned mk = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        mk |= (live[rb] && ci[d] < cn[d] && bs[d] - j >= 0 && bs[d] - j < g.in[d]) ? (1u << j) : 0u;
      vm[rb][d] = mk;
    }
    lin[rb] = (bs[0] * g.in[1] + bs[1]) * g.in[2] + bs[2];
  }

  f4v acc[8][RB][NB];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[c][rb][nb] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  // the sample's region tensor (and addend): out-of-range offsets read 0
  const size_t rvol_in = (size_t)g.in[0] * g.in[1] * g.in[2];
  const Rsrc rs = make_rsrc(x + (size_t)b * rvol_in * CI, (uint32_t)(rvol_in * CI * 4));
  Rsrc rs2;
  if constexpr (X2) rs2 = make_rsrc(x2 + (size_t)b * rvol_in * CI, (uint32_t)(rvol_in * CI * 4));

  // ---- K loop: tap rows grouped by the input row they read ----
  constexpr int kRowOrder[9][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}, {0, 2}, {1, 2}, {2, 0}, {2, 1}, {2, 2}};
  f4v a[RB][2][CB];   // the live input row: voxels x = c (0), c - 1 (1), all channel blocks
#pragma unroll
  for (int it = 0; it < 9; ++it) {
    const int tz = kRowOrder[it][0], ty = kRowOrder[it][1];
    const int jz = tz >> 1, jy = ty >> 1;
    if (it == 0 || it == 4 || it == 6 || it == 8) {   // a new input row (jz, jy): each voxel loaded once
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int jx = 0; jx < 2; ++jx) {
          const bool ok = ((vm[rb][0] >> jz) & (vm[rb][1] >> jy) & (vm[rb][2] >> jx) & 1u) != 0;
          const uint32_t vo = (uint32_t)(lin[rb] - jz * sz - jy * sy - jx) * (uint32_t)(CI * 4) + (uint32_t)kq * 16u;
#pragma unroll
          for (int cb = 0; cb < CB; ++cb) {
            const uint32_t eo = ok ? vo + (uint32_t)cb * 64u : kOob;
            f4v v = ld4(rs, eo, 0);
            if constexpr (X2) v += ld4(rs2, eo, 0);
            a[rb][jx][cb] = v;
          }
        }
    }
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
      const int c4 = cb * 16 + kq * 4;
      f4v bw[3][NB];
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const float* wt = w + (size_t)((tz * 3 + ty) * 3 + tx) * CO * CI;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          bw[tx][nb] = *reinterpret_cast<const f4v*>(wt + (size_t)(nb * 16 + m) * CI + c4);
      }
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int cls = ((tz & 1) << 2) | ((ty & 1) << 1) | (tx & 1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
              acc[cls][rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][tx >> 1][cb][s], bw[tx][nb][s],
                                                                      acc[cls][rb][nb], 0, 0, 0);
      }
    }
  }

  // ---- epilogue: eval BN + ReLU; acc[cls][rb][nb][r] = (cell 4 kq + r of the row block, channel nb * 16 + m),
  // class (pz, py, px) = bits (2, 1, 0): output 2 c - P + par per dim, masked to the output region ----
  const size_t rvol = (size_t)g.stn[0] * g.stn[1] * g.stn[2];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    // x of the lane's first output (cell 4 kq, px = 0) in the region; its run [lo, hi) of the 8
    const int vx0 = 2 * (cf[2] + xb[rb] * 16 + kq * 4) - g.pad[2] - g.o0[2];
    const int lo = vx0 < 0 ? -vx0 : 0, hi = g.on[2] - vx0 < 8 ? g.on[2] - vx0 : 8;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int co = nb * 16 + m;
      const float sc = bn_scale ? bn_scale[co] : 1.0f, sh = bn_scale ? bn_shift[co] : 0.0f,
                  mu = bn_scale ? bn_mean[co] : 0.0f;
#pragma unroll
      for (int pzy = 0; pzy < 4; ++pzy) {
        const int vz = 2 * (cf[0] + lz[rb]) + (pzy >> 1) - g.pad[0] - g.o0[0];
        const int vy = 2 * (cf[1] + ly[rb]) + (pzy & 1) - g.pad[1] - g.o0[1];
        if (!live[rb] || vz < 0 || vz >= g.on[0] || vy < 0 || vy >= g.on[1] || lo >= hi) continue;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          float t = acc[pzy * 2 + (i & 1)][rb][nb][i >> 1];
          if (bn_scale) t = fmaxf((t - mu) * sc + sh, 0.0f);
          v[i] = t;
        }
        // element index of v[0] in the stored box (signed: v[0] may lie before the row's first voxel)
        const long vox = ((long)(vz + g.st0[0]) * g.stn[1] + (vy + g.st0[1])) * g.stn[2] + (vx0 + g.st0[2]);
        if (g.out_cf) {
          const long e = (long)(((size_t)b * CO + co) * rvol) + vox;
          float* p = y + e;
          switch ((int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) {
            case 0: store_run8<0>(p, v, lo, hi); break;
            case 1: store_run8<1>(p, v, lo, hi); break;
            case 2: store_run8<2>(p, v, lo, hi); break;
            default: store_run8<3>(p, v, lo, hi); break;
          }
        } else {
          float* p = y + ((long)((size_t)b * rvol) + vox) * CO + co;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (i >= lo && i < hi) p[(long)i * CO] = v[i];
        }
      }
    }
  }
}

// 32 -> 16 (deconv_2_0): two row blocks per wave, 148 VGPRs with the addend / 160 without, no scratch, three
// waves per SIMD (four row blocks: 240-248 VGPRs, two waves).  64 -> 32 (deconv_3_0) stays on the class
// kernel: its region is small (25 x 17 x 21 cells at cfg 2) and a cell wave carries all 27 taps' weights
// (27 x 4 x 2 float4 loads per 16 cells), so its few long waves are bound by their own load latency -- in
// the cfg-2 eval step 0.226 ms (one row block, both column blocks per wave) and 0.260 ms (two row blocks,
// the column blocks split over two waves) against the class kernel's 0.195 ms
constexpr int kCellsRB = 2;

template <int CI, int CO, int RB>
void launch_t2_cells(const float* x, const float* x2, const float* w, float* y, const float* sc, const float* sh,
                     const float* mu, int B, const Geo& g, hipStream_t s) {
  const dim3 grid = cell_grid(RB, B, g.o0, g.on, g.pad);
  if (x2)
    hipLaunchKernelGGL((conv3d_t2_cells_kernel<CI, CO, RB, true>), grid, dim3(kBlock), 0, s, x, x2, w, y, sc, sh, mu, g);
  else
    hipLaunchKernelGGL((conv3d_t2_cells_kernel<CI, CO, RB, false>), grid, dim3(kBlock), 0, s, x, x2, w, y, sc, sh, mu, g);
}

template <int V>
using Const = std::integral_constant<int, V>;
template <int... U, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, U...>, F&& f) {
  (f(Const<U>{}), ...);
}

// the cell kernel's sub-steps in order: input rows (iz, iy) ascending, channel blocks, then the cell's outputs
// (dz, dy) whose tap (iz - 2 dz, iy - 2 dy) lies in the 3 x 3 window -- CZ CY 9 CB of them
template <int CZ, int CY, int CB>
struct S2CellSteps {
  static constexpr int kSubs = CZ * CY * 9 * CB;
  // sub-step u's (step, dz, dy), packed: found by enumeration
  static constexpr int find(int u) {
    int k = 0;
    for (int st = 0; st < (2 * CZ + 1) * (2 * CY + 1) * CB; ++st) {
      const int iz = st / ((2 * CY + 1) * CB), iy = st / CB % (2 * CY + 1);
      for (int dz = 0; dz < CZ; ++dz)
        for (int dy = 0; dy < CY; ++dy) {
          const int tz = iz - 2 * dz, ty = iy - 2 * dy;
          if (tz < 0 || tz > 2 || ty < 0 || ty > 2) continue;
          if (k++ == u) return (st * CZ + dz) * CY + dy;
        }
    }
    return -1;
  }
  static constexpr int step(int u) { return find(u) / (CZ * CY); }
  static constexpr int dz(int u) { return find(u) / CY % CZ; }
  static constexpr int dy(int u) { return find(u) % CY; }
};

// ---- stride-2 convolutions, register-tiled z x y output cells (conv_1_0) ----
// In the per-lane kernel above every output fetches its own 3 x 3 input rows (tz, ty): the row the outputs
// y' and y' + 1 share, and the plane z' and z' + 1 share, are loaded again by another wave, often another
// workgroup -- 9 input rows per output, and whether the repeats hit L2 is timing.  Here a GEMM row is a CELL of
// CZ x CY outputs in (z, y) at one output x: its outputs read the (2 CZ + 1) x (2 CY + 1) input rows
// 2 o - P + t of the cell's first output o, so the lane loads each of them once (the three x taps together,
// per 16-channel block, the per-lane kernel's loads) and feeds every accumulator that reads the row with the
// weights of its own tap (tz, ty) = (iz - 2 dz, iy - 2 dy) -- 25 / 4 rows per output for 2 x 2 cells.  No LDS,
// no barriers.  Rows are the flattened (cell-z, cell-y, x) index of the output region, 16 consecutive rows an
// MFMA row block, RB row blocks per wave (they share the weight loads); only an odd extent in z or y leaves
// half-empty cells (computed, not stored).  Each lane has its own base voxel and per-dim masks of the input
// rows / x taps that exist in the (boxed) volume, as region_conv: a missing input reads 0 through kOob.
// Order: input rows ascending (iz, iy); per accumulator that is ascending (tz, ty), then channel block, then
// tx, then K-step -- region_conv<kS2>'s products in region_conv<kS2>'s order, with the same zero operands:
// every output is bit-equal to the per-lane kernel's.
template <int CI, int CO, int CZ, int CY, int RB, int QM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void conv3d_s2_cells_kernel(
    const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
    const float* __restrict__ bn_scale, const float* __restrict__ bn_shift, const float* __restrict__ bn_mean,
    Geo g) {
  constexpr int NB = CO / 16, CB = CI / 16, NZ = 2 * CZ + 1, NY = 2 * CY + 1;
  static_assert(CI % 16 == 0 && CO % 16 == 0, "channel counts in multiples of 16");
  static_assert(QM == 0 || QM == 1, "the fp32 volume: NCDHW or channel quads");
  const int lane = (int)threadIdx.x & 63;
  const int m = lane & 15, kq = lane >> 4;
  const int b = (int)blockIdx.z;

  const int ncy = (g.on[1] + CY - 1) / CY;
  const int rows = ((g.on[0] + CZ - 1) / CZ) * ncy * g.on[2];
  const int bx = xcd_work_id((int)blockIdx.x, (int)gridDim.x);
  const int row0 = (bx * (kBlock / 64) + ((int)threadIdx.x >> 6)) * (16 * RB);
  if (row0 >= rows) return;   // wave-uniform; no barriers in this kernel

  // per row block: the input voxel of the cell's first output's tap (0, 0, 0) in the addressed box (linear,
  // may be negative: masked) and, per dim, which of the cell's input rows / x taps exist
  int lin[RB];
  unsigned vm[RB][3];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int r = row0 + rb * 16 + m;
    const bool ok = r < rows;
    const int rr = ok ? r : 0;
    const int jx = rr % g.on[2], c = rr / g.on[2];
    const int o[3] = {g.o0[0] + (c / ncy) * CZ, g.o0[1] + (c % ncy) * CY, g.o0[2] + jx};
    constexpr int cnt[3] = {NZ, NY, 3};
    int bs[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      bs[d] = 2 * o[d] - g.pad[d] - g.i0[d];   // taps off the box: off the volume
      unsigned mk = 0;
#pragma unroll
      for (int i = 0; i < cnt[d]; ++i) mk |= (ok && bs[d] + i >= 0 && bs[d] + i < g.in[d]) ? (1u << i) : 0u;
      vm[rb][d] = mk;
    }
    lin[rb] = (bs[0] * g.in[1] + bs[1]) * g.in[2] + bs[2];
  }

  f4v acc[CZ * CY][RB][NB];
#pragma unroll
  for (int c = 0; c < CZ * CY; ++c)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[c][rb][nb] = f4v{0.0f, 0.0f, 0.0f, 0.0f};

  const size_t rvol = (size_t)g.in[0] * g.in[1] * g.in[2];   // voxels of the (boxed) volume per plane
  const int sy = g.in[2], sz = g.in[1] * g.in[2];
  // ---- K loop, software-pipelined by hand (left to itself the scheduler hoists every load of the unrolled
  // loop and spills): a STEP is an input row (iz, iy) and channel block -- its three x taps, loaded once; a
  // SUB-STEP is one accumulator (dz, dy) reading it, with its own tap row's weights.  The next step's inputs
  // and the next sub-step's weights are issued ahead of the current sub-step's MFMAs, and nothing moves
  // across a sub-step's end ----
  using T = S2CellSteps<CZ, CY, CB>;
  f4v a[2][3][RB], bw[2][3][NB];
  auto load_a = [&](auto step) {   // step st = (iz * NY + iy) * CB + cb
    constexpr int st = decltype(step)::value, iz = st / (NY * CB), iy = st / CB % NY, cb = st % CB;
    // the sample's 4 channel quads / 16 channel planes of this block: out-of-range offsets read 0
    const Rsrc rs = QM == 1 ? make_rsrc(x + ((size_t)b * (CI / 4) + cb * 4) * rvol * 4, (uint32_t)(rvol * 64))
                            : make_rsrc(x + ((size_t)b * CI + cb * 16) * rvol, (uint32_t)(rvol * 64));
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const bool ok = ((vm[rb][0] >> iz) & (vm[rb][1] >> iy) & (vm[rb][2] >> tx) & 1u) != 0;
        const uint32_t vx = (uint32_t)(lin[rb] + iz * sz + iy * sy + tx);
        if constexpr (QM == 1) {   // the quad (c4 / 4) of the voxel: one 16-byte load
          a[st & 1][tx][rb] = ld4(rs, ok ? ((uint32_t)kq * (uint32_t)rvol + vx) * 16u : kOob, 0);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q)
            a[st & 1][tx][rb][q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                rs, (int)(ok ? ((uint32_t)(kq * 4 + q) * (uint32_t)rvol + vx) * 4u : kOob), 0, 0));
        }
      }
  };
  auto load_w = [&](auto sub) {   // sub-step u: tap row (tz, ty) = (iz - 2 dz, iy - 2 dy), w[tap][co][ci]
    constexpr int u = decltype(sub)::value, st = T::step(u);
    constexpr int tz = st / (NY * CB) - 2 * T::dz(u), ty = st / CB % NY - 2 * T::dy(u);
    // (a tap row's weights are read by CZ CY sub-steps far apart: the lane's offset goes through an empty asm
    // so that the compiler loads them again instead of keeping all 27 taps' weights in registers)
    int wo = m * CI + kq * 4;
    asm volatile("" : "+v"(wo));
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const float* wt = w + (size_t)((tz * 3 + ty) * 3 + tx) * CO * CI + (st % CB) * 16;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) bw[u & 1][tx][nb] = *reinterpret_cast<const f4v*>(wt + nb * 16 * CI + wo);
    }
  };
  load_a(Const<0>{});
  load_w(Const<0>{});
  static_for(std::make_integer_sequence<int, T::kSubs>{}, [&](auto sub) {   // (compile-time u: registers only)
    constexpr int u = decltype(sub)::value, st = T::step(u), c = T::dz(u) * CY + T::dy(u);
    if constexpr (u + 1 < T::kSubs) load_w(Const<u + 1>{});
    if constexpr ((u == 0 || T::step(u > 0 ? u - 1 : 0) != st) && st + 1 < NZ * NY * CB) load_a(Const<st + 1>{});
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            acc[c][rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st & 1][tx][rb][s], bw[u & 1][tx][nb][s],
                                                                  acc[c][rb][nb], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  });

  // ---- epilogue: eval BN + ReLU; acc[cell output][rb][nb][r] = (row kq * 4 + r of the row block, channel
  // nb * 16 + m), masked to the region (the clipped last cells in z and y) ----
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int co = nb * 16 + m;
    const float sc = bn_scale ? bn_scale[co] : 1.0f, sh = bn_scale ? bn_shift[co] : 0.0f,
                mu = bn_scale ? bn_mean[co] : 0.0f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + rb * 16 + kq * 4 + r;
        if (row >= rows) continue;
        const int jx = row % g.on[2], c = row / g.on[2];
#pragma unroll
        for (int dz = 0; dz < CZ; ++dz)
#pragma unroll
          for (int dy = 0; dy < CY; ++dy) {
            const int vz = (c / ncy) * CZ + dz, vy = (c % ncy) * CY + dy;
            if (vz >= g.on[0] || vy >= g.on[1]) continue;
            float v = acc[dz * CY + dy][rb][nb][r];
            if (bn_scale) v = fmaxf((v - mu) * sc + sh, 0.0f);
            store_out(y, g, b, co, vz, vy, jx, CO, v);
          }
      }
  }
}

// 2 x 2 cells, two row blocks per wave: 155 VGPRs from channel quads, 162 from NCDHW, no scratch, three waves per
// SIMD (the attribute above holds the compiler to them).  The row blocks share each sub-step's weight loads, and
// that is what decides: at cfg 2 conv_1_0 alone takes 1.15 ms on the per-lane kernel, 1.00 ms here, and 1.28 /
// 1.31 / 1.30 ms with one row block per wave and cells of 2 x 2 / 2 x 4 / 4 x 4 (97 / 117 / 151 VGPRs) -- fewer
// input loads but one set of weight loads per 12 MFMAs instead of per 24; 2 x 4 cells with two row blocks spill
// 
constexpr int kS2CellZ = 2, kS2CellY = 2, kS2CellRB = 2;

template <int CI, int CO>
void launch_s2_cells(const float* x, int in_c4, const float* w, float* y, const float* sc, const float* sh,
                     const float* mu, int B, const Geo& g, hipStream_t s) {
  const dim3 grid = s2_cell_grid(kS2CellZ, kS2CellY, kS2CellRB, B, g.on);
  if (in_c4)
    hipLaunchKernelGGL((conv3d_s2_cells_kernel<CI, CO, kS2CellZ, kS2CellY, kS2CellRB, 1>), grid, dim3(kBlock), 0, s,
                       x, w, y, sc, sh, mu, g);
  else
    hipLaunchKernelGGL((conv3d_s2_cells_kernel<CI, CO, kS2CellZ, kS2CellY, kS2CellRB, 0>), grid, dim3(kBlock), 0, s,
                       x, w, y, sc, sh, mu, g);
}

}  // namespace

int launch_conv3d_region(int mode, bool out_cf, int in_c4, const float* x, const float* x2, const float* w,
                         float* y, int B, int CI, int CO, const int* n, const int* o0, const int* on, const int* i0,
                         const int* in, const int* pad, const float* bn_scale, const float* bn_shift,
                         const float* bn_mean, hipStream_t s, const uint32_t* absmax, uint32_t* y_bound,
                         bool per_lane, const int* st0, const int* stn, bool s2_lds) {
  Geo g;
  g.y_bound = y_bound;
  g.out_cf = out_cf ? 1 : 0;
  g.in_c4 = in_c4;
  g.absmax = absmax;
  for (int d = 0; d < 3; ++d) {
    g.n[d] = n[d];
    g.o0[d] = o0[d];
    g.on[d] = on[d];
    g.i0[d] = i0 ? i0[d] : 0;
    g.in[d] = in ? in[d] : n[d];
    g.pad[d] = pad ? pad[d] : 1;
    g.st0[d] = st0 ? st0[d] : 0;
    g.stn[d] = stn ? stn[d] : on[d];
  }
  // Which kernel runs is a function of the arguments alone (the flags per_lane and s2_lds; no environment).
  // Two variants were measured slower and were removed in this commit: an LDS-staged fp32 stride-1 kernel
  // (conv_1_1 0.42 against 0.34 ms alone, the fp32 eval step 6.60 against 5.94 ms) and four row blocks per wave
  // for S2 from the channel-quad volume.
  // conv_1_0 (S2 32 -> 16) from the whole fp32 volume: the LDS-staged kernel with the flag MVS_CONV_S2_LDS
  // (opt-in, slower in the step: conv3d_s2_lds.hip)
  if (mode == kS2 && CI == 32 && CO == 16 && (in_c4 == 0 || in_c4 == 1) && !x2 && !absmax && !y_bound &&
      !per_lane && !st0 && !stn && !i0 && !in && !out_cf && pad && s2_lds &&
      (uint64_t)n[0] * (uint64_t)n[1] * (uint64_t)n[2] * 128u < 0xFFFFFFF0ull) {   // (32-bit byte offsets)
    launch_conv_s2_lds(x, in_c4, w, y, B, n, o0, on, pad, bn_scale, bn_shift, bn_mean, s);
    return MVS_OK;
  }
  // conv_1_0 (S2 32 -> 16) from the fp32 volume, either layout, boxed or whole, any store box: the cell kernel
  // (bit-equal to the per-lane kernel); the per-lane kernel with per_lane, with bound words (the slot a maximum
  // lands in follows its wave numbering), for the bf16 / split volumes and for every other shape
  if (mode == kS2 && s2_cells_shape(CI, CO) && (in_c4 == 0 || in_c4 == 1) && !x2 && !absmax && !y_bound && !per_lane)
    return launch_s2_cells<32, 16>(x, in_c4, w, y, bn_scale, bn_shift, bn_mean, B, g, s), MVS_OK;
// two row blocks per wave (one and four measured slower on the cfg-2 eval and train-mode steps)
#define MVS_REGION_CASE(MD, A, C)                                                       \
  if (mode == MD && CI == A && CO == C) {                                               \
    launch_mode<MD, A, C, 2>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s);        \
    return MVS_OK;                                                                      \
  }
#define MVS_REGION_S2(A, C)                                                                                   \
  if (mode == kS2 && CI == A && CO == C) {                                                                    \
    if (in_c4 == 3) launch_mode<kS2, A, C, 2, 3>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s);         \
    else if (in_c4 == 2) launch_mode<kS2, A, C, 2, 2>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s);    \
    else if (in_c4) launch_mode<kS2, A, C, 2, 1>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s);         \
    else launch_mode<kS2, A, C, 2, 0>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s);                    \
    return MVS_OK;                                                                                            \
  }
  // S2: conv_1_0 / conv_2_0 / conv_3_0 (32 -> 16 / 32 / 64); S1: conv_k_1; T2: deconv_3_0 (64 -> 32),
  // deconv_2_0 (32 -> 16)
  MVS_REGION_S2(32, 16) MVS_REGION_S2(32, 32) MVS_REGION_S2(32, 64)
  MVS_REGION_CASE(kS1, 16, 16) MVS_REGION_CASE(kS1, 32, 32) MVS_REGION_CASE(kS1, 64, 64)
  // transposed 32 -> 16: the cell kernel (one pass per input cell, bit-equal to the class kernel; either
  // layout, one or two inputs, any store box); the class kernel with per_lane (the autograd forward, tests),
  // for 64 -> 32 (measured faster there, above), for an empty region, and with bound words: which of their
  // slots a maximum lands in follows the class kernel's wave numbering (bound_update), and
  // tests/golden/region_conv_pins.json pins those bytes; the fp32 eval chain asks for none
  if (mode == kT2 && CI == 32 && CO == 16 && !per_lane && !y_bound && on[0] > 0 && on[1] > 0 && on[2] > 0)
    return launch_t2_cells<32, 16, kCellsRB>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s), MVS_OK;
  // the class kernel: four row blocks per wave for deconv_2_0 (32 -> 16: 0.323 -> 0.302 ms at cfg 2), two
  // for deconv_3_0 (64 -> 32: equal).  Per-output accumulation order does not depend on the row blocks
  if (mode == kT2 && CI == 32 && CO == 16)
    return launch_mode<kT2, 32, 16, 4>(x, x2, w, y, bn_scale, bn_shift, bn_mean, B, g, s), MVS_OK;
  MVS_REGION_CASE(kT2, 64, 32)
#undef MVS_REGION_CASE
#undef MVS_REGION_S2
  return MVS_ERR_INVALID_ARGUMENT;
}

int conv3d_s2_cells_geometry(int CI, int CO, const int* on, long long* out) {
  out[0] = kS2CellZ;
  out[1] = kS2CellY;
  out[2] = kS2CellRB;
  out[3] = s2_cell_rows(kS2CellZ, kS2CellY, on);
  out[4] = s2_cell_waves(kS2CellZ, kS2CellY, kS2CellRB, on);
  out[5] = s2_cell_grid(kS2CellZ, kS2CellY, kS2CellRB, 1, on).x;
  return s2_cells_shape(CI, CO) ? 1 : 0;
}

// Input gradient of the stacked stride-2 convolution (conv_1_0 / conv_2_0 / conv_3_0: 32 -> 112 on the output
// box `out` of the whole volume n): gx[b][ci][i] = sum over taps t and co of gy[b][(i + pad_lo - t) / 2][co]
// w[co][ci][t] -- the transposed mode with gy (channels-last, 112 channels) as the input region at origin 0,
// the whole volume as the output region, written NCDHW, w27 [27][32][112], four partial sums per output.
void launch_conv3d_s2_dgrad(const float* gy, const float* w27, float* gx, int B, const int* n, const int* pad_lo,
                            const int* out, hipStream_t s) {
  Geo g;
  g.y_bound = nullptr;
  g.absmax = nullptr;
  g.out_cf = 1;
  g.in_c4 = 0;
  for (int d = 0; d < 3; ++d) {
    g.n[d] = n[d];
    g.o0[d] = 0;
    g.on[d] = n[d];
    g.i0[d] = 0;
    g.in[d] = out[d];
    g.pad[d] = pad_lo[d];
    g.st0[d] = 0;
    g.stn[d] = n[d];
  }
  launch_mode<kT2, 112, 32, 2, 0, 4>(gy, nullptr, w27, gx, nullptr, nullptr, nullptr, B, g, s);
}

// Input gradient of a transposed region convolution (deconv_3_0 64 -> 32, deconv_2_0 32 -> 16: input voxel i
// reaches box outputs 2 i - crop + t): gx[b][i][ci] = sum over taps t and co of gy[b][2 i - crop + t][co]
// w[ci][co][t] -- the stride-2 mode with gy (channels-last, CF = 32 or 16 channels, the box `out`) as the volume,
// pad = crop, no tap flip, x's extent `in` as the output box, written channels-last, w27 [27][CC][CF], one partial
// sum per tap plane.
int launch_conv3d_t2_dgrad(const float* gy, const float* w27, float* gx, int B, int CC, int CF, const int* in,
                           const int* crop, const int* out, hipStream_t s) {
  Geo g;
  g.y_bound = nullptr;
  g.absmax = nullptr;
  g.out_cf = 0;
  g.in_c4 = 0;
  for (int d = 0; d < 3; ++d) {
    g.n[d] = out[d];
    g.o0[d] = 0;
    g.on[d] = in[d];
    g.i0[d] = 0;
    g.in[d] = out[d];
    g.pad[d] = crop[d];
    g.st0[d] = 0;
    g.stn[d] = in[d];
  }
  if (CC == 64 && CF == 32) launch_mode<kS2, 32, 64, 2, 4, 3>(gy, nullptr, w27, gx, nullptr, nullptr, nullptr, B, g, s);
  else if (CC == 32 && CF == 16)
    launch_mode<kS2, 16, 32, 2, 4, 3>(gy, nullptr, w27, gx, nullptr, nullptr, nullptr, B, g, s);
  else return MVS_ERR_INVALID_ARGUMENT;
  return MVS_OK;
}

}  // namespace mvs
