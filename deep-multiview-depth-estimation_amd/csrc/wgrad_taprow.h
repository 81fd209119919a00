// wgrad_taprow.h -- the plan the region layers' weight-gradient kernels share (conv3d_region_wgrad.hip: stride 1;
// conv3d_s2_wgrad.hip: stacked stride 2; conv3d_t2_wgrad.hip: deconv_3_0 / deconv_2_0; deconv3d_region_bwd.hip:
// deconv_1_0), on the f32-input matrix cores.
//
// Per tap t the weight gradient is a GEMM whose K runs over the voxels of the grid the taps are counted from
// (the output voxels of a convolution, the input voxels of a transposed one): A = one operand read as
// [voxel][row channel], B = the other read as [voxel shifted by t][column channel].
//   * The 27 taps are partitioned over workgroups by tap row (tz, ty): a workgroup owns the row's three x taps.
//   * A workgroup is persistent over a K chunk: kTapRowChunks chunks per tap row, chunk c walks the tiles c,
//     c + chunks, ... (taprow_walk) and keeps its accumulators in registers across every tile of the chunk.
//   * A tile is TR rows (flattened b, z, y) x kTapRowTX x-voxels.  Per tile the workgroup writes the element
//     offsets of the tile's rows in both operands into an LDS table (64-bit: the operands pass 2^32 bytes at the
//     training shapes; -1: no such row, or its tap row is off the other operand), stages both operands in LDS
//     once (channels-last operands: one 16-byte global load per 4 channels into padded voxel records; what is
//     past an extent reads 0, its products vanish) and runs the K-steps of 4 consecutive x-voxels as
//     v_mfma_f32_16x16x4_f32.
//   * Each wave stores its blocks into the partial [27][R][C] slot of its (chunk, K part): every slot entry is
//     written exactly once per launch, none relies on a zeroed workspace.  wgrad_reduce_kernel sums the slots in
//     slot order (deterministic, no atomics) into dw[r][c][27].
// Products and sums are fp32 (each MFMA step an fmaf chain).
//
// The invariant the multi-pass and the past-2^32-bytes tests protect lives here: the tile loop and its barriers
// are workgroup-uniform (tile, chunk and chunks depend on blockIdx / gridDim only), every slot entry is written
// once, row and sample addresses are 64-bit.  What differs between the kernels -- the wave-to-block mapping, the
// MFMA packing, record pitches and their bank reasoning, the layouts read in place -- is in their files.
// Everything here is __forceinline__ with compile-time sizes: no call survives into the ISA.
#pragma once
#include "common.h"
#include "packed.h"

namespace mvs {

constexpr int kTapRowTX = 16;        // x-voxels of a tile
constexpr int kTapRowChunks = 168;   // K chunks: x 9 tap rows = 1512 workgroups, just under 3 rounds of the 512
                                     // that fit 256 CUs at two (<= 80 KB of LDS) per CU
// the stride-2 pairing (conv3d_s2_wgrad.hip, conv3d_t2_wgrad.hip): of the fine-grid row that meets a tile's 16
// coarse voxels, voxel j is staged as record (j & 1) * kTapRowHX + (j >> 1) -- 17 even then 17 odd records -- so
// the four coarse voxels of a K-step (fine voxels two apart) read adjacent records: tap tx = 0 even record k,
// tx = 1 odd record k, tx = 2 even record k + 1
constexpr int kTapRowHX = kTapRowTX + 1;   // staged fine records per parity (even: taps 0 and 2)
constexpr int kTapRowFR = 2 * kTapRowHX;   // staged fine records per row

// ---- host geometry ----
struct TapRowGeo {
  int rows;              // flattened (b, z, y) rows of the K grid
  int tiles_x, tiles;    // x tiles per row group, tiles in all
};

inline TapRowGeo taprow_geo(int rows, int nx, int TR) {
  TapRowGeo t;
  t.rows = rows;
  t.tiles_x = (nx + kTapRowTX - 1) / kTapRowTX;
  t.tiles = t.tiles_x * ((rows + TR - 1) / TR);
  return t;
}

// workgroups per tap row; a launch has chunks * KP partial slots
inline int taprow_chunks(const TapRowGeo& t) { return t.tiles < kTapRowChunks ? t.tiles : kTapRowChunks; }

inline size_t taprow_workspace_bytes(const TapRowGeo& t, int KP, int slot_floats) {
  return (size_t)taprow_chunks(t) * KP * slot_floats * sizeof(float);
}

inline dim3 taprow_grid(const TapRowGeo& t) { return dim3(9u * (unsigned)taprow_chunks(t)); }

// ---- device: the workgroup's tap row and K chunk ----
struct TapRowBlock {
  int row_tap, tz, ty;   // tap row 3 tz + ty
  int chunk, chunks;
};

__device__ __forceinline__ TapRowBlock taprow_block() {
  TapRowBlock b;
  b.row_tap = (int)blockIdx.x % 9, b.chunk = (int)blockIdx.x / 9, b.chunks = (int)gridDim.x / 9;
  b.tz = b.row_tap / 3, b.ty = b.row_tap % 3;
  return b;
}

template <int N>
__device__ __forceinline__ void taprow_zero(f4v (&acc)[3][N]) {
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < N; ++c) acc[tx][c] = f4v{0.0f, 0.0f, 0.0f, 0.0f};
}

// The chunk's tile walk.  Per tile: rows(R, oa, ob) gives the element offsets of row R < t.rows in the two
// operands (left at -1: none), thread r < TR filling entry r of the table; tile(x0, rowa, rowb) stages the tile at
// x-voxel x0 and runs its K-steps (its own barrier between the two).
template <int TR, class Rows, class Tile>
__device__ __forceinline__ void taprow_walk(const TapRowBlock& b, const TapRowGeo& t, Rows&& rows, Tile&& tile_body) {
  __shared__ long long rowa[TR], rowb[TR];   // element offsets of the tile's rows (-1: no such row)
  const int tid = (int)threadIdx.x, chunk = b.chunk, chunks = b.chunks;
  for (int tile = chunk; tile < t.tiles; tile += chunks) {   // workgroup-uniform
    const int x0 = (tile % t.tiles_x) * kTapRowTX, row0 = (tile / t.tiles_x) * TR;
    __syncthreads();   // the previous tile's operand reads are done
    if (tid < TR) {
      const int R = row0 + tid;
      long long oa = -1, ob = -1;
      if (R < t.rows) rows(R, oa, ob);
      rowa[tid] = oa;
      rowb[tid] = ob;
    }
    __syncthreads();
    tile_body(x0, rowa, rowb);
  }
}

// ---- device: staging ----
// ROWS channels-last rows of NX voxels from x-voxel x0 on into records of P floats (record r * NX + xi): items
// (voxel, 16-byte chunk), chunk fastest (coalesced loads); voxels at or past nx read 0.  row[r]: the row's element
// offset.  SKIP: rows with live[r] < 0 are not staged at all (the K-steps skip them; their records keep what the
// previous tile left); otherwise a row with row[r] < 0 is staged as zeros.
template <int C, int P, int ROWS, int NX, bool SKIP>
__device__ __forceinline__ void taprow_stage_rows(float* lds, const float* __restrict__ src, const long long* row,
                                                  const long long* live, int x0, int nx) {
  constexpr int Q = C / 4;   // 16-byte chunks per voxel
  for (int e = (int)threadIdx.x; e < ROWS * NX * Q; e += kBlock) {
    const int c4 = e % Q, v = e / Q;
    const int r = v / NX, xi = v % NX;
    if (SKIP && live[r] < 0) continue;
    const long long o = row[r];
    f4v val{0.0f, 0.0f, 0.0f, 0.0f};
    if ((SKIP || o >= 0) && x0 + xi < nx) val = *reinterpret_cast<const f4v*>(src + o + (long long)(x0 + xi) * C + 4 * c4);
    *reinterpret_cast<f4v*>(lds + v * P + 4 * c4) = val;
  }
}

// The fine rows of ROWS coarse rows, channels-last, the kTapRowFR voxels fx0 + j (fx0 may be negative) in parity
// order: items (row, fine voxel j, chunk), chunk fastest; voxels off [0, nx) read 0; rows with row[r] < 0 are not
// staged.
template <int C, int P, int ROWS>
__device__ __forceinline__ void taprow_stage_parity_rows(float* lds, const float* __restrict__ src,
                                                         const long long* row, int fx0, int nx) {
  constexpr int Q = C / 4;
  for (int e = (int)threadIdx.x; e < ROWS * kTapRowFR * Q; e += kBlock) {
    const int c4 = e % Q, t = e / Q;
    const int j = t % kTapRowFR, r = t / kTapRowFR;
    const long long o = row[r];
    if (o < 0) continue;
    const int fx = fx0 + j;
    f4v val{0.0f, 0.0f, 0.0f, 0.0f};
    if (fx >= 0 && fx < nx) val = *reinterpret_cast<const f4v*>(src + o + (long long)fx * C + 4 * c4);
    *reinterpret_cast<f4v*>(lds + (r * kTapRowFR + (j & 1) * kTapRowHX + (j >> 1)) * P + 4 * c4) = val;
  }
}

// ---- device: the K-steps of one staged row ----
// a: the row's A records (pitch PA) at this lane's (kq, channel) offset; b: the same of its B records (pitch PB).
// Per step of 4 voxels NCB A values (channel blocks 16 apart) meet the three x taps' B values: stride 1, tap tx is
// record 4 s + tx; stride 2, the parity order above.
template <int STRIDE, int NCB, int PA, int PB, int N>
__device__ __forceinline__ void taprow_ksteps(const float* a, const float* b, f4v (&acc)[3][N]) {
  static_assert(NCB <= N && (STRIDE == 1 || STRIDE == 2), "accumulator blocks");
#pragma unroll
  for (int s = 0; s < kTapRowTX / 4; ++s) {
    float av[NCB], bv[3];
#pragma unroll
    for (int c = 0; c < NCB; ++c) av[c] = a[4 * s * PA + c * 16];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) bv[tx] = b[(4 * s + (STRIDE == 1 ? tx : (tx & 1) * kTapRowHX + (tx >> 1))) * PB];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx)
#pragma unroll
      for (int c = 0; c < NCB; ++c)
        acc[tx][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bv[tx], acc[tx][c], 0, 0, 0);
  }
}

// ---- device: the slot store ----
// acc[tx][c][i] = D[row channel (rb0 + c) * 16 + 4 kq + i][column channel nb * 16 + m] of tap 3 row_tap + tx into
// the partial slot [27][R][C]; blocks c >= ncb are not the wave's
template <int R, int C, int N>
__device__ __forceinline__ void taprow_store_slot(float* slot, int row_tap, int rb0, int ncb, int nb, int lane,
                                                  const f4v (&acc)[3][N]) {
  const int m = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int c = 0; c < N; ++c) {
      if (c >= ncb) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        slot[((size_t)(row_tap * 3 + tx) * R + (rb0 + c) * 16 + 4 * kq + i) * C + nb * 16 + m] = acc[tx][c][i];
    }
}

// ---- the reduce ----
namespace {

// dw[r][c][t] = the slots' [t][r][c] entries summed in slot order (fixed: deterministic)
__global__ __launch_bounds__(kBlock) void wgrad_reduce_kernel(const float* __restrict__ part, int slots, int R, int C,
                                                             float* __restrict__ dw) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);   // (t, r, c): consecutive lanes, consecutive c
  const int n = 27 * R * C;
  if (i >= n) return;
  float s = 0.0f;
  for (int k = 0; k < slots; ++k) s += part[(size_t)k * n + i];
  const int c = i % C, r = (i / C) % R, t = i / (C * R);
  dw[((size_t)r * C + c) * 27 + t] = s;
}

inline void launch_wgrad_reduce(const float* part, int slots, int R, int C, float* dw, hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((27 * R * C + kBlock - 1) / kBlock), dim3(kBlock), 0, s, part, slots, R,
                     C, dw);
}

}  // namespace

}  // namespace mvs
