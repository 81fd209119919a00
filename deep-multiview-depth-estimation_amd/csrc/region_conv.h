// region_conv.h -- what the regulariser's region convolutions share (conv3d_region.hip: fp32 MFMA;
// conv3d_region_split.hip: split-fp16 MFMA; conv2d_split.hip: the split-record LDS tile only): the mode
// constants and the out-of-range offset, the parity-class geometry, the launch grids, the swizzled
// split-record tile and the K-32 product.  Everything is __forceinline__ or constexpr: no call survives
// into the ISA, and the kernels' code is what the inline copies compiled to.
#pragma once
#include "common.h"
#include "packed.h"
#include "split.h"

namespace mvs {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));
// out-of-range buffer offset for taps / voxels without input (the loads return 0; + 16 stays out of
// range); every descriptor built on it covers less than 2^32 - 64 bytes (the C entry points check)
constexpr uint32_t kOob = 0xFFFFFFC0u;
constexpr int kS1 = 0, kS2 = 1, kT2 = 2;

// ---- row geometry ----
// T2 parity class: per dim, outputs o with (o + P) % 2 == par; first such o in the region and count
__device__ __forceinline__ void class_dim(int o0, int on, int p, int par, int& first, int& cnt) {
  first = o0 + (((o0 + p) & 1) != par ? 1 : 0);
  cnt = first < o0 + on ? (o0 + on - 1 - first) / 2 + 1 : 0;
}

// T2 cells: output o belongs to cell (o + P) >> 1, which holds the outputs 2 c - P and 2 c - P + 1 (parity 0
// and 1 of o + P) and reads the inputs c - 1 (tap 2, parity 0 only) and c (taps 0 / 1).  First cell with an
// output in [o0, o0 + on) and the count of such cells; on >= 1
__host__ __device__ __forceinline__ void cell_dim(int o0, int on, int p, int& first, int& cnt) {
  first = (o0 + p) >> 1;
  cnt = ((o0 + on - 1 + p) >> 1) - first + 1;
}

// ---- launch grids (multiples of the 8 XCDs: xcd_work_id) ----
// the per-lane kernels: (row chunks of the largest parity class / of the region) x classes x batch
inline dim3 region_grid(int mode, int RB, int B, const int* on) {
  const bool t2 = mode == kT2;
  const long rows = (long)(t2 ? (on[0] + 1) / 2 : on[0]) * (t2 ? (on[1] + 1) / 2 : on[1]) *
                    (t2 ? (on[2] + 1) / 2 : on[2]);
  const long per_block = (kBlock / 64) * 16 * RB;
  return dim3(xcd_grid((int)((rows + per_block - 1) / per_block)).x, t2 ? 8u : 1u, (unsigned)B);
}

// the T2 cell kernel: (16-cell row blocks of every cell line, RB per wave) x batch
inline dim3 cell_grid(int RB, int B, const int* o0, const int* on, const int* pad) {
  int cf[3], cn[3];
  for (int d = 0; d < 3; ++d) cell_dim(o0[d], on[d], pad[d], cf[d], cn[d]);
  const long blocks = (long)cn[0] * cn[1] * ((cn[2] + 15) / 16);
  const long waves = (blocks + RB - 1) / RB, per_block = kBlock / 64;
  return dim3(xcd_grid((int)((waves + per_block - 1) / per_block)).x, 1u, (unsigned)B);
}

// the S2 cell kernel: a GEMM row is a cell of CZ x CY outputs in (z, y) at one output x; rows = the flattened
// (cell-z, cell-y, x) index, 16 consecutive rows an MFMA row block, RB row blocks per wave.  The (c_in, c_out)
// it is instantiated for, which are the ones launch_conv3d_region sends to it
constexpr bool s2_cells_shape(int CI, int CO) { return CI == 32 && CO == 16; }

inline long s2_cell_rows(int CZ, int CY, const int* on) {
  return (long)((on[0] + CZ - 1) / CZ) * ((on[1] + CY - 1) / CY) * on[2];
}

inline long s2_cell_waves(int CZ, int CY, int RB, const int* on) {
  return (s2_cell_rows(CZ, CY, on) + 16 * RB - 1) / (16 * RB);
}

inline dim3 s2_cell_grid(int CZ, int CY, int RB, int B, const int* on) {
  const long per_block = kBlock / 64;
  return dim3(xcd_grid((int)((s2_cell_waves(CZ, CY, RB, on) + per_block - 1) / per_block)).x, 1u, (unsigned)B);
}

// the LDS-staged kernels: tiles x batch
inline dim3 tile_grid(int tiles, int B) { return dim3(xcd_grid(tiles).x, (unsigned)B); }

// ---- the split-record LDS tile: one record per voxel / pixel, CI hi then CI lo fp16, its 16-byte
// chunks XOR-swizzled by voxel so the 16 lanes of an MFMA row group (16 consecutive voxels) hit 16
// distinct bank groups ----
template <int CI>
struct SplitRec {
  static constexpr int REC = CI * 4;     // bytes per record
  static constexpr int NCH = REC / 16;   // 16-byte chunks per record: 2 .. 16
  __device__ __forceinline__ static int chunk_off(int v, int c) {
    return v * REC + ((c ^ ((v / (16 / NCH)) % NCH)) << 4);
  }
};

// ---- one K-32 step ----
// x_hi w_hi + x_hi w_lo + x_lo w_hi into one accumulator (each product exact in fp32; the dropped
// x_lo w_lo is below 2^-22 of the product)
__device__ __forceinline__ void mfma3(const h8v& ahi, const h8v& alo, const h8v& bhi, const h8v& blo, f4v& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bhi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, blo, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bhi, acc, 0, 0, 0);
}

// this lane's part (0 hi, 1 lo) of the weight fragment wf[kb][nb][part][lane] of K block kb, column block nb
__device__ __forceinline__ h8v wfrag(const h8v* __restrict__ wf, int kb, int NB, int nb, int part, int lane) {
  return wf[((size_t)(kb * NB + nb) * 2 + part) * 64 + lane];
}

}  // namespace mvs
