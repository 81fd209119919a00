// conv2d_bwd.hip -- input and weight gradients of the 2-D feature encoder's and refinement net's bias-free
// Conv2d layers under autograd (model.py:22-65 FeatureEncoder, model.py:134-145 refinement; forward:
// conv2d_narrow.hip), fp32 NCHW read in place, the weight [c_out][c_in][k][k] as the module stores it, padding
// k / 2, the eight (c_in, c_out, k, stride) of conv2d_narrow.hip.  Every offset into x, gy and gx is a size_t.
//
// Input gradient (conv2d_dgrad_kernel), a gather without atomics:
//   gx[n][ci][iy][ix] = sum_{co, ky, kx} w[co][ci][ky][kx] * gy[n][co][oy][ox],  oy * S + ky - P = iy (x alike)
// A 256-thread workgroup owns 8 rows x 64 columns of input pixels of one image; a thread owns two pixels of one
// row and all c_in channels of both in registers.  Per pass the gy halo of the tile (10 rows, zero outside the
// image) is staged in LDS for NC output channels, as the forward stages x, beside those channels' weights
// transposed to [co][ky][kx][ci] (one 16-byte broadcast read per four FMAs of each pixel).
//   stride 1 (3 x 3): the pixels are columns lx and lx + 32 of the tile (bank-conflict-free halo reads, and the
//     two share every weight); three taps per axis.
//   stride 2 (5 x 5): only the taps of the pixel's parity contribute.  The row parity PY is blockIdx.z, so it is
//     workgroup-uniform and a template argument of the body: rows 2 j + PY take ky = 2 a + PY, a < 3 - PY, from
//     output row j + 1 - a.  The thread's pixels are columns 2 j and 2 j + 1: the column parity is the pixel
//     index, a compile-time constant of the unrolled FMA chain (kx = 2 b + p, b < 3 - p, output column j + 1 - b).
//     No branch depends on the thread.
// Sums are fp32 fmaf chains in the order co, ky, kx.
//
// Weight gradient (conv2d_wgrad_kernel + conv2d_wgrad_reduce_kernel), the scheme of conv3d_wgrad.hip on
// v_mfma_f32_16x16x4_f32 (exact fp32 products and sums):
//   gw[co][ci][ky][kx] = sum_{n, oy, ox} gy[n][co][oy][ox] * x[n][ci][oy * S + ky - P][ox * S + kx - P]
// per input channel a GEMM with M = the k * k taps (one or two 16-row blocks; rows past k * k are dropped),
// N = c_out (one or two 16-column blocks; columns past c_out are fed zeros) and K = the output pixels.  A
// persistent workgroup walks 32 x 8 output tiles (tile, tile + grid, ...: workgroup-uniform): the tile's gy
// (c_out x 256 values, zero past the output) is staged in LDS once, then per pass the x halo blocks of four input
// channels (zero outside the image), one channel per wave; a wave runs the tile's 64 K-steps of 4 consecutive
// output columns, its accumulators per channel in registers across every tile it visits.  Each workgroup stores one
// slot [c_in][RB * 16][NB * 16], every entry written exactly once per launch; the reduce kernel sums the slots in
// slot order into gw.  Nothing is zeroed and there are no atomics: the result is bit-reproducible whatever the
// workspace held.
// Padding to the MFMA block: a wave whose channel is past c_in (c_in = 3) has its halo block staged as zeros
// without a load and stores nothing; lanes past c_out read gy row 0 of the LDS tile and feed 0; rows past k * k
// read the last tap's LDS address.  No padded lane reads global memory.
//
// wgrad_taprow.h is not used: its plan partitions 27 taps into nine tap rows of three with both operands
// channels-last in voxel records, and its reduce kernel and slot layout are [27][R][C] -> dw[r][c][27].  Here
// the taps are 9 or 25, both operands are NCHW planes, and a slot is [c_in][taps][c_out]; what is kept is its
// conventions: persistent workgroups, one slot per workgroup written once, a slot-order reduce.
//
// Built without packed fp32 (mvs_amd/_build.py SOURCE_FLAGS), as bn_train_bwd.hip is: both kernels keep LDS
// stores (the staging of the next pass) beside fp32 arithmetic in one loop, the pattern DESIGN.md §3.7 found
// miscompiled with v_pk_*_f32.  The input gradient's chains are scalar fmaf per channel either way and the weight
// gradient's arithmetic is MFMA, so nothing is lost.
#include "launchers.h"
#include "packed.h"

namespace mvs {
namespace {

constexpr int kDTY = 8;     // input rows of an input-gradient tile
constexpr int kDLX = 32;    // threads per row; two pixels each
constexpr int kDHH = kDTY + 2;
static_assert(kBlock == kDLX * kDTY, "input gradient: thread (threadIdx.x / kDLX, threadIdx.x % kDLX) of a tile");

constexpr int dgrad_pass_channels(int cout, int per_co) {
  // output channels per pass: the largest divisor of cout up to 16 whose weights stay within 4608 floats
  int nc = 1;
  for (int d = 1; d <= cout && d <= 16; ++d)
    if (cout % d == 0 && d * per_co <= 4608) nc = d;
  return nc;
}

template <int CIN, int COUT, int K, int S>
struct DgradCfg {
  static constexpr int KK = K * K;
  static constexpr int CP = (CIN + 3) & ~3;                 // c_in padded to 16-byte weight records
  static constexpr int HW = (S == 1 ? 2 * kDLX : kDLX) + 2; // halo columns
  static constexpr int kPlane = kDHH * HW;
  static constexpr int NC = dgrad_pass_channels(COUT, KK * CP);
  static constexpr int kG = NC * kPlane, kW = NC * KK * CP;
};

// one workgroup's tile; PY: the row parity (stride 2)
template <int CIN, int COUT, int K, int S, int PY>
__device__ __forceinline__ void dgrad_tile(const float* __restrict__ gy, const float* __restrict__ w,
                                           float* __restrict__ gx, int H, int W, int Ho, int Wo, int tiles_x,
                                           float* gs, float* ws) {
  using C = DgradCfg<CIN, COUT, K, S>;
  constexpr int KK = C::KK, CP = C::CP, HW = C::HW, kPlane = C::kPlane, NC = C::NC;
  constexpr int TA = S == 1 ? 3 : 3 - PY;   // taps per row of this parity
  constexpr int kUA = CP >= 32 ? 1 : TA;    // c_in = 32: one tap row's weight records in flight, not three (VGPRs)
  const int tile = (int)blockIdx.x, n = (int)blockIdx.y;
  const int lx = (int)threadIdx.x % kDLX, ly = (int)threadIdx.x / kDLX;
  // stride 1: input pixel (row0 + ly, col0 + lx + 32 p); stride 2: (2 (row0 + ly) + PY, 2 (col0 + lx) + p).  The halo
  // starts at output (row0 - 1, col0 - 1) either way.
  const int col0 = (tile % tiles_x) * (S == 1 ? 2 * kDLX : kDLX), row0 = (tile / tiles_x) * kDTY;
  const size_t oplane = (size_t)Ho * Wo;
  const float* gb = gy + (size_t)n * COUT * oplane;

  float acc[2][CP];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[p][c] = 0.0f;

  for (int q = 0; q < COUT / NC; ++q) {
    __syncthreads();   // the previous pass's reads are done
    for (int e = (int)threadIdx.x; e < C::kG; e += kBlock) {
      const int c = e / kPlane, r = e % kPlane;
      const int oy = row0 - 1 + r / HW, ox = col0 - 1 + r % HW;
      gs[e] = (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo)
                  ? gb[(size_t)(q * NC + c) * oplane + (size_t)oy * Wo + ox]
                  : 0.0f;
    }
    for (int e = (int)threadIdx.x; e < C::kW; e += kBlock) {
      const int ci = e % CP, t = (e / CP) % KK, c = e / (CP * KK);
      ws[e] = ci < CIN ? w[((size_t)(q * NC + c) * CIN + ci) * KK + t] : 0.0f;
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
#pragma unroll kUA
      for (int a = 0; a < TA; ++a) {
        const int ky = S == 1 ? a : 2 * a + PY;
        const float* gr = gs + c * kPlane + (ly + 2 - a) * HW + lx + 2;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          // stride 1: both pixels take kx = b (output column pixel + 1 - b); stride 2: pixel p takes kx = 2 b + p
          // from output column j + 1 - b, b < 3 - p
          const float g0 = gr[-b];
          const float g1 = S == 1 ? gr[kDLX - b] : g0;
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            if (S == 2 && b >= 3 - p) continue;
            const int kx = S == 1 ? b : 2 * b + p;
            const f4v* wp = reinterpret_cast<const f4v*>(ws + ((c * K + ky) * K + kx) * CP);
            const float g = p == 0 ? g0 : g1;
#pragma unroll
            for (int c4 = 0; c4 < CP / 4; ++c4) {
              const f4v w4 = wp[c4];
#pragma unroll
              for (int j = 0; j < 4; ++j) acc[p][4 * c4 + j] = fmaf(w4[j], g, acc[p][4 * c4 + j]);
            }
          }
        }
      }
    }
  }

  const int iy = S == 1 ? row0 + ly : 2 * (row0 + ly) + PY;
  if (iy >= H) return;
  const size_t plane = (size_t)H * W;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int ix = S == 1 ? col0 + lx + kDLX * p : 2 * (col0 + lx) + p;
    if (ix >= W) continue;
    float* ob = gx + (size_t)n * CIN * plane + (size_t)iy * W + ix;
#pragma unroll
    for (int c = 0; c < CIN; ++c) ob[(size_t)c * plane] = acc[p][c];
  }
}

template <int CIN, int COUT, int K, int S>
__global__ __launch_bounds__(kBlock) void conv2d_dgrad_kernel(const float* __restrict__ gy,
                                                             const float* __restrict__ w, float* __restrict__ gx,
                                                             int H, int W, int Ho, int Wo, int tiles_x) {
  using C = DgradCfg<CIN, COUT, K, S>;
  __shared__ float gs[C::kG];
  __shared__ __attribute__((aligned(16))) float ws[C::kW];
  if (S == 1 || blockIdx.z == 0)   // workgroup-uniform
    dgrad_tile<CIN, COUT, K, S, 0>(gy, w, gx, H, W, Ho, Wo, tiles_x, gs, ws);
  else
    dgrad_tile<CIN, COUT, K, S, 1>(gy, w, gx, H, W, Ho, Wo, tiles_x, gs, ws);
}

// ---- weight gradient ----
constexpr int kGTX = 32, kGTY = 8;
constexpr int kGPix = kGTX * kGTY;     // 256 output pixels per tile
constexpr int kGyPitch = kGPix + 4;    // B-operand rows: lanes (kq, co) on banks 4 co + kq
constexpr int kWgradBlocks = 512;      // persistent workgroups (2 per CU: <= 54 KB of LDS each)
constexpr int kGWaves = 4;             // input channels staged per pass, one per wave
static_assert(kBlock == kGWaves * 64, "weight gradient: wave w takes halo block w of a pass (channel 4 p + w)");

template <int CIN, int COUT, int K, int S>
struct WgradCfg {
  static constexpr int KK = K * K;
  static constexpr int RB = (KK + 15) / 16, NB = (COUT + 15) / 16;
  static constexpr int NP = (CIN + kGWaves - 1) / kGWaves;   // passes of 4 channels, one per wave
  static constexpr int IH = (kGTY - 1) * S + K, IW = (kGTX - 1) * S + K;
  static constexpr int kStage = IH * IW;
  static constexpr int kSlot = CIN * RB * 16 * NB * 16;
};

template <int CIN, int COUT, int K, int S>
__global__ __launch_bounds__(kBlock) void conv2d_wgrad_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ gy,
                                                             float* __restrict__ part, int N, int H, int W, int Ho,
                                                             int Wo, int tiles_x, int tiles_y) {
  using C = WgradCfg<CIN, COUT, K, S>;
  constexpr int KK = C::KK, RB = C::RB, NB = C::NB, NP = C::NP, IW = C::IW, kStage = C::kStage, P = K / 2;
  __shared__ float xs[kGWaves * kStage];
  __shared__ float gys[COUT * kGyPitch];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int m16 = lane & 15, kq = lane >> 4;
  // A operand: lane (m16, kq) supplies tap rb * 16 + m16 (clamped: rows >= k * k are dropped) of output pixel
  // 4 xg + kq of its wave's channel
  int toff[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const int t = min(rb * 16 + m16, KK - 1);
    toff[rb] = wave * kStage + (t / K) * IW + (t % K) + kq * S;
  }
  // B operand: lane (kq, m16) supplies gy[co = nb * 16 + m16][pixel 4 xg + kq] (0 for co >= c_out)
  bool bon[NB];
  int boff[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    bon[nb] = nb * 16 + m16 < COUT;
    boff[nb] = (bon[nb] ? nb * 16 + m16 : 0) * kGyPitch + kq;
  }
  f4v acc[NP][RB][NB];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[p][rb][nb] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
  const size_t plane = (size_t)H * W, oplane = (size_t)Ho * Wo;
  const int total = N * tiles_y * tiles_x;
  for (int tile = (int)blockIdx.x; tile < total; tile += (int)gridDim.x) {   // workgroup-uniform
    int t = tile;
    const int ox0 = (t % tiles_x) * kGTX;
    t /= tiles_x;
    const int oy0 = (t % tiles_y) * kGTY;
    const int n = t / tiles_y;
    __syncthreads();   // the previous tile's reads are done
    const float* gb = gy + (size_t)n * COUT * oplane;
    for (int e = (int)threadIdx.x; e < COUT * kGPix; e += kBlock) {
      const int co = e / kGPix, v = e % kGPix;
      const int ox = ox0 + v % kGTX, oy = oy0 + v / kGTX;
      gys[co * kGyPitch + v] = (ox < Wo && oy < Ho) ? gb[(size_t)co * oplane + (size_t)oy * Wo + ox] : 0.0f;
    }
    const int iy0 = oy0 * S - P, ix0 = ox0 * S - P;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      if (p > 0) __syncthreads();   // the previous pass's A reads are done
      const float* xb = x + ((size_t)n * CIN + 4 * p) * plane;
      for (int e = (int)threadIdx.x; e < kGWaves * kStage; e += kBlock) {
        const int u = e / kStage, r = e % kStage;
        const int iy = iy0 + r / IW, ix = ix0 + r % IW;
        xs[e] = (4 * p + u < CIN && iy >= 0 && iy < H && ix >= 0 && ix < W)
                    ? xb[(size_t)u * plane + (size_t)iy * W + ix]
                    : 0.0f;
      }
      __syncthreads();
#pragma unroll 2
      for (int ly = 0; ly < kGTY; ++ly) {
        const int abase = ly * S * IW, bbase = ly * kGTX;
#pragma unroll
        for (int xg = 0; xg < kGTX / 4; ++xg) {
          float bv[NB], av[RB];
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const float v = gys[boff[nb] + bbase + 4 * xg];
            bv[nb] = bon[nb] ? v : 0.0f;
          }
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) av[rb] = xs[toff[rb] + abase + 4 * xg * S];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
              acc[p][rb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rb], bv[nb], acc[p][rb][nb], 0, 0, 0);
        }
      }
    }
  }
  // slot [c_in][RB * 16 rows][NB * 16 cols]: acc[p][rb][nb][r] = D[row rb * 16 + 4 kq + r][col nb * 16 + m16] of
  // channel 4 p + wave
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int ci = 4 * p + wave;
    if (ci >= CIN) continue;   // wave-uniform
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          part[(((size_t)blockIdx.x * CIN + ci) * (RB * 16) + rb * 16 + 4 * kq + r) * (NB * 16) + nb * 16 + m16] =
              acc[p][rb][nb][r];
  }
}

// gw[co][ci][t] = the slots' [ci][t][co] entries summed in slot order (fixed: deterministic)
__global__ __launch_bounds__(kBlock) void conv2d_wgrad_reduce_kernel(const float* __restrict__ part, int slots,
                                                                    int cin, int cout, int kk, int rows, int cols,
                                                                    float* __restrict__ dw) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= cout * cin * kk) return;
  const int t = i % kk, ci = (i / kk) % cin, co = i / (kk * cin);
  float s = 0.0f;
  for (int g = 0; g < slots; ++g) s += part[(((size_t)g * cin + ci) * rows + t) * cols + co];
  dw[i] = s;
}

int out_len(int n, int K, int S) { return (n + 2 * (K / 2) - K) / S + 1; }

template <int CIN, int COUT, int K, int S>
void launch_dgrad(const float* gy, const float* w, float* gx, int N, int H, int W, hipStream_t s) {
  const int Ho = out_len(H, K, S), Wo = out_len(W, K, S);
  const int cols = S == 1 ? W : (W + 1) / 2, rows = S == 1 ? H : (H + 1) / 2;
  const int tiles_x = (cols + (S == 1 ? 2 * kDLX : kDLX) - 1) / (S == 1 ? 2 * kDLX : kDLX);
  const int tiles_y = (rows + kDTY - 1) / kDTY;
  hipLaunchKernelGGL((conv2d_dgrad_kernel<CIN, COUT, K, S>), dim3((unsigned)(tiles_x * tiles_y), (unsigned)N, S),
                     dim3(kBlock), 0, s, gy, w, gx, H, W, Ho, Wo, tiles_x);
}

template <int CIN, int COUT, int K, int S>
void launch_wgrad(const float* x, const float* gy, float* part, float* dw, int N, int H, int W, int slots,
                  hipStream_t s) {
  using C = WgradCfg<CIN, COUT, K, S>;
  const int Ho = out_len(H, K, S), Wo = out_len(W, K, S);
  const int tiles_x = (Wo + kGTX - 1) / kGTX, tiles_y = (Ho + kGTY - 1) / kGTY;
  hipLaunchKernelGGL((conv2d_wgrad_kernel<CIN, COUT, K, S>), dim3((unsigned)slots), dim3(kBlock), 0, s, x, gy, part,
                     N, H, W, Ho, Wo, tiles_x, tiles_y);
  const int n = COUT * CIN * K * K;
  hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, part, slots, CIN,
                     COUT, K * K, C::RB * 16, C::NB * 16, dw);
}

}  // namespace

// FeatureEncoder (model.py:22-65) and the refinement net (model.py:134-145): conv2d_narrow.hip's list
#define MVS_CONV2D_BWD_SHAPES(X) \
  X(3, 8, 3, 1) X(8, 8, 3, 1) X(8, 16, 5, 2) X(16, 16, 3, 1) X(16, 32, 5, 2) X(32, 32, 3, 1) X(4, 32, 3, 1) X(32, 1, 3, 1)

bool conv2d_bwd_supported(int Cin, int Cout, int K, int stride) {
#define MVS_CASE(A, C, KK, SS) \
  if (Cin == A && Cout == C && K == KK && stride == SS) return true;
  MVS_CONV2D_BWD_SHAPES(MVS_CASE)
#undef MVS_CASE
  return false;
}

Conv2dWgradPlan conv2d_wgrad_plan(int N, int Cin, int Cout, int H, int W, int K, int stride) {
  Conv2dWgradPlan p{0, 0, 0};
  const int Ho = out_len(H, K, stride), Wo = out_len(W, K, stride);
  const long tiles = (long)N * ((Ho + kGTY - 1) / kGTY) * ((Wo + kGTX - 1) / kGTX);
  p.tiles = (int)tiles;
  p.slots = (int)(tiles < kWgradBlocks ? tiles : kWgradBlocks);
  p.slot_floats = Cin * ((K * K + 15) / 16) * 16 * ((Cout + 15) / 16) * 16;
  return p;
}

int launch_conv2d_dgrad(const float* gy, const float* w, float* gx, int N, int Cin, int Cout, int H, int W, int K,
                        int stride, hipStream_t s) {
#define MVS_CASE(A, C, KK, SS)                                     \
  if (Cin == A && Cout == C && K == KK && stride == SS) {          \
    launch_dgrad<A, C, KK, SS>(gy, w, gx, N, H, W, s);             \
    return MVS_OK;                                                 \
  }
  MVS_CONV2D_BWD_SHAPES(MVS_CASE)
#undef MVS_CASE
  return MVS_ERR_INVALID_ARGUMENT;
}

int launch_conv2d_wgrad(const float* x, const float* gy, int N, int Cin, int Cout, int H, int W, int K, int stride,
                        float* part, float* dw, hipStream_t s) {
  const int slots = conv2d_wgrad_plan(N, Cin, Cout, H, W, K, stride).slots;
#define MVS_CASE(A, C, KK, SS)                                        \
  if (Cin == A && Cout == C && K == KK && stride == SS) {             \
    launch_wgrad<A, C, KK, SS>(x, gy, part, dw, N, H, W, slots, s);   \
    return MVS_OK;                                                    \
  }
  MVS_CONV2D_BWD_SHAPES(MVS_CASE)
#undef MVS_CASE
  return MVS_ERR_INVALID_ARGUMENT;
}

}  // namespace mvs
