// capi.hip -- the C ABI declared in include/mvs_cost_volume.h (drop-in boundary, SURVEY.md §8 b).
//
// Validates arguments, lays out the caller-provided workspace and enqueues the launchers of the
// other translation units on the caller's stream.  No allocation, no synchronisation, no global
// mutable state: every entry point is re-entrant per stream and graph-capturable.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "../../include/eval/mvs_region_launch.h"
#include "../../include/fusion/mvs_cloud_eval.h"
#include "../../include/fusion/mvs_depth_filter.h"
#include "../../include/fusion/mvs_view_fusion.h"
#include "../../include/train/mvs_loss.h"
#include "../../include/train/mvs_region_train.h"
#include "launchers.h"

namespace {

using mvs::Geometry;

// store_es: output element bytes of the packed (2 <= V <= 8) fused kernel this geometry feeds
// (element_bytes(CvStore)), 0 for entry points that build no cost-volume store descriptors
int check_geometry(int B, int V, int C, int h, int w, int d_count, Geometry& g, int store_es = 0) {
  if (B <= 0 || C <= 0 || h < 2 || w < 2 || d_count <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (V < 1 || V > MVS_MAX_VIEWS) return MVS_ERR_UNSUPPORTED_VIEWS;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  // per-image plane offsets are 32-bit; work ids are 32-bit ints; packed corners are 16-bit
  if ((uint64_t)C * hw >= (1ull << 31) || h > 32000 || w > 32000) return MVS_ERR_TOO_LARGE;
  // the packed kernels build 32-bit buffer descriptors and offsets: a sample's padded channel-quad
  // images (V * ceil(C/4) * (h+2) * (w+2) float4, byte offsets held in ints) and a plane group's
  // cost-volume run (up to 8 planes * hw * store_es bytes: the store offsets soff0 + pl * hw * es)
  const bool packed = V >= 2 && V <= 8;
  const uint64_t padded = (uint64_t)V * (uint64_t)((C + 3) / 4) * (uint64_t)(h + 2) * (uint64_t)(w + 2) * 16u;
  if (packed && (padded >= (1ull << 31) || 8ull * hw * (uint64_t)store_es >= (1ull << 32))) return MVS_ERR_TOO_LARGE;
  const uint64_t tiles = (hw + mvs::kBlock - 1) / mvs::kBlock;
  const uint64_t total = (uint64_t)B * tiles * (uint64_t)d_count;
  if (total >= (1ull << 31) - 8) return MVS_ERR_TOO_LARGE;
  g.B = B;
  g.V = V;
  g.C = C;
  g.h = h;
  g.w = w;
  g.Dc = d_count;
  g.tiles = (int)tiles;
  g.total = (int)total;
  return MVS_OK;
}

bool cams_ok(const float* K, const float* R, const float* T, const float* d_min, const float* d_int) {
  return K && R && T && d_min && d_int;
}

// BN scale, shift and mean come as a triple or not at all
bool bn_all_or_none(const float* a, const float* b, const float* c) {
  return !((a != nullptr) != (b != nullptr) || (a != nullptr) != (c != nullptr));
}

// two pointers that come as a pair or not at all
bool both_or_neither(const void* p, const void* q) { return (p != nullptr) == (q != nullptr); }

// a weight / operand scale exponent split_scale() can have produced
bool exp_ok(int e) { return e >= -120 && e <= 120; }

// the box origin + [0, size) lies inside the outputs of conv3d(k 3, stride 2, padding pad) over n:
// (n + 2 pad - 3) / 2 + 1 per dim
bool s2_region_ok(int origin, int size, int n, int pad) { return origin + size <= (n + 2 * pad - 3) / 2 + 1; }

// The split-fp16 weight scale (csrc/split.h): 2^ew with max|w| 2^ew < 2^14, clamped to [-120, 120];
// all-zero weights: ew = 0.  false on a non-finite weight.
bool split_scale(const float* w, size_t n, int* ew) {
  float m = 0.0f;
  for (size_t k = 0; k < n; ++k) {
    if (!std::isfinite(w[k])) return false;
    m = std::max(m, std::fabs(w[k]));
  }
  int e = 0;
  if (m > 0.0f) (void)std::frexp(m, &e);
  *ew = m > 0.0f ? std::min(std::max(14 - e, -120), 120) : 0;
  return true;
}

// The split of a scaled weight (csrc/split.h): hi = fp16(v), lo = fp16(v - hi), as bit patterns.
struct SplitBits { uint16_t hi, lo; };
SplitBits split_bits(float v) {
  const _Float16 hi = (_Float16)v;
  const _Float16 lo = (_Float16)(v - (float)hi);
  SplitBits b;
  std::memcpy(&b.hi, &hi, 2);
  std::memcpy(&b.lo, &lo, 2);
  return b;
}

// The cost-volume store of the fused warp + variance kernels
enum class CvStore { kF32, kBf16, kQuadF32, kQuadSplit, kQuadBf16 };

// channel-quad layout [B][C/4][D][h][w][4] (else NCDHW)
bool is_quad(CvStore s) { return s == CvStore::kQuadF32 || s == CvStore::kQuadSplit || s == CvStore::kQuadBf16; }

// bytes per stored element: an fp32 / bf16 value, or a quad of them (the split quad: 4 hi + 4 lo fp16)
int element_bytes(CvStore s) {
  switch (s) {
    case CvStore::kF32: return 4;
    case CvStore::kBf16: return 2;
    case CvStore::kQuadBf16: return 8;
    case CvStore::kQuadF32:
    case CvStore::kQuadSplit: return 16;
  }
  return 0;   // not reached: every store kind is named above (-Wswitch flags a missing one)
}

// Fused warp + variance into the cost volume ``store`` describes.
int cost_volume_fwd_impl(const float* feat, const float* K, const float* R, const float* T,
                         const float* d_min, const float* d_int, int batch_size, int n_views,
                         int channels, int h, int w, int d_begin, int d_count, float d_scale,
                         float* workspace, void* cv_out, CvStore store, void* stream, void* ev0, void* ev1,
                         uint32_t* absmax = nullptr) {
  if (!feat || !workspace || !cv_out) return MVS_ERR_INVALID_ARGUMENT;
  Geometry g;
  int st = check_geometry(batch_size, n_views, channels, h, w, d_count, g, element_bytes(store));
  if (st != MVS_OK) return st;
  if (!cams_ok(K, R, T, d_min, d_int) || d_begin < 0) return MVS_ERR_INVALID_ARGUMENT;
  const mvs::LaunchCheck lc;
  hipStream_t s = (hipStream_t)stream;
  if (n_views == 1) {  // the variance of a single view is identically zero (0 in fp32 and bf16)
    if (absmax && hipMemsetAsync(absmax, 0, 8 * sizeof(uint32_t), s) != hipSuccess) return MVS_ERR_HIP;
    st = mvs_plane_sampling(K, R, T, d_min, d_int, batch_size, n_views, h, w, d_begin, d_count,
                            d_scale, workspace, stream);
    if (st != MVS_OK) return st;
    const size_t ch = is_quad(store) ? (size_t)((channels + 3) / 4) : (size_t)channels;
    if (hipMemsetAsync(cv_out, 0, (size_t)batch_size * ch * d_count * h * w * element_bytes(store), s) != hipSuccess)
      return MVS_ERR_HIP;
    return lc.status();
  }
  float* packed = reinterpret_cast<float*>(
      reinterpret_cast<char*>(workspace) +
      mvs::align256((size_t)batch_size * n_views * d_count * 9 * sizeof(float)));
  const mvs::Cams cm{K, R, T, d_min, d_int, d_begin, d_scale};
  hipEvent_t e0 = (hipEvent_t)ev0, e1 = (hipEvent_t)ev1;
  switch (store) {
    case CvStore::kF32:
      mvs::launch_cost_volume_fwd(g, feat, cm, workspace, packed, static_cast<float*>(cv_out), s, e0, e1);
      break;
    case CvStore::kQuadF32:
    case CvStore::kQuadSplit:
      mvs::launch_cost_volume_fwd_c4(g, feat, cm, workspace, packed, static_cast<float*>(cv_out), s, e0, e1, absmax,
                                     store == CvStore::kQuadSplit);
      break;
    case CvStore::kQuadBf16:
      mvs::launch_cost_volume_fwd_c4_bf16(g, feat, cm, workspace, packed, cv_out, s, e0, e1);
      break;
    case CvStore::kBf16:
      mvs::launch_cost_volume_fwd_bf16(g, feat, cm, workspace, packed, cv_out, s, e0, e1);
      break;
  }
  return lc.status();
}


// ---- training extension (include/train/mvs_region_train.h): what its entry points share ----
// every pointer non-null and 16-byte aligned
template <class... P>
bool aligned16(const P*... p) {
  return (... && (p != nullptr)) && !((... | (uintptr_t)p) & 15u);
}

// MVS_OK when mvs_conv3d_region_wgrad can launch on this geometry
int region_wgrad_geometry(int batch, int channels, const int* in_size) {
  if (!in_size || batch <= 0 || !mvs::conv3d_region_wgrad_supported(channels)) return MVS_ERR_INVALID_ARGUMENT;
  uint64_t vox = (uint64_t)batch;
  for (int k = 0; k < 3; ++k) {
    if (in_size[k] < 3) return MVS_ERR_INVALID_ARGUMENT;
    vox *= (uint64_t)in_size[k];
    if (vox >= (1ull << 31)) return MVS_ERR_TOO_LARGE;   // 32-bit row and tile indices
  }
  return MVS_OK;
}

// MVS_OK when the weight / input gradient of a stride-2 layer can launch: a coarse and a fine grid with fine
// index 2 c - offset + t (the stride-2 convolution: its output box and the volume, offset = pad_lo; the transposed
// ones: their input and the output box, offset = crop; null where the caller has none: not checked), gy on the
// fine grid or the coarse one with gy_channels channels
int stride2_bwd_geometry(int batch, const int* coarse, const int* fine, const int* offset, bool gy_fine,
                         int gy_channels) {
  if (!coarse || !fine || batch <= 0) return MVS_ERR_INVALID_ARGUMENT;
  const int* gy_size = gy_fine ? fine : coarse;
  uint64_t cvox = (uint64_t)batch, fvox = (uint64_t)batch, gy_sample = 1;
  for (int k = 0; k < 3; ++k)
    if (coarse[k] < 1 || fine[k] < 1 || (offset && offset[k] < 0)) return MVS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 3; ++k) {
    cvox *= (uint64_t)coarse[k];
    fvox *= (uint64_t)fine[k];
    gy_sample *= (uint64_t)gy_size[k];
    if (cvox >= (1ull << 31) || fvox >= (1ull << 31)) return MVS_ERR_TOO_LARGE;   // 32-bit row and voxel indices
    // 2 c - offset + t in 32 bits (a coarse gy extent this long also fails the sample bound below: no status of
    // the stride-2 convolution's entry points, which never tested it here, changes)
    if (coarse[k] >= (1 << 29) || (offset && offset[k] >= (1 << 29))) return MVS_ERR_TOO_LARGE;
  }
  // one sample of gy behind one 32-bit buffer descriptor (the input gradient's loads)
  if (gy_sample * (uint64_t)gy_channels * sizeof(float) >= 0xFFFFFFC0ull) return MVS_ERR_TOO_LARGE;
  return MVS_OK;
}

int s2_region_bwd_geometry(int batch, const int* dims, const int* pad_lo, const int* out_size) {
  return stride2_bwd_geometry(batch, out_size, dims, pad_lo, false, 112);
}

int t2_region_bwd_geometry(int batch, int c_in, int c_out, const int* in_size, const int* crop, const int* out_size) {
  if (!mvs::conv3d_t2_wgrad_supported(c_in, c_out)) return MVS_ERR_INVALID_ARGUMENT;
  return stride2_bwd_geometry(batch, in_size, out_size, crop, true, c_out);
}

int deconv3d_bwd_geometry(int batch, int c_in, int c_out, const int* in_size, const int* crop, const int* out_size) {
  if (c_in != 16 || c_out != 8) return MVS_ERR_INVALID_ARGUMENT;
  return stride2_bwd_geometry(batch, in_size, out_size, crop, true, c_out);
}

// MVS_OK when the 2-D convolutions' weight / input gradient can launch: a shape with kernels, element counts of x and
// gy below 2^31 (32-bit tile and staging indices; offsets are 64-bit)
int conv2d_bwd_geometry(int n, int c_in, int c_out, int h, int w, int k, int stride) {
  if (n <= 0 || h <= 0 || w <= 0 || !mvs::conv2d_bwd_supported(c_in, c_out, k, stride)) return MVS_ERR_INVALID_ARGUMENT;
  const uint64_t ho = (uint64_t)((h + 2 * (k / 2) - k) / stride + 1), wo = (uint64_t)((w + 2 * (k / 2) - k) / stride + 1);
  // (factor by factor: no product of two of these passes 2^64)
  const uint64_t lim = 1ull << 31, hw = (uint64_t)h * (uint64_t)w, ohw = ho * wo;
  if (hw >= lim || hw * (uint64_t)c_in >= lim || hw * (uint64_t)c_in * (uint64_t)n >= lim) return MVS_ERR_TOO_LARGE;
  if (ohw >= lim || ohw * (uint64_t)c_out >= lim || ohw * (uint64_t)c_out * (uint64_t)n >= lim) return MVS_ERR_TOO_LARGE;
  return MVS_OK;
}

// the entry points' prologue and epilogue: `ok` (pointers, flags), then the geometry's status, then (the input
// gradients: grid.z) the batch bound, then the launch under a LaunchCheck
template <class Launch>
int train_launch(bool ok, int geometry, bool batch_in_grid_z, int batch, Launch&& launch) {
  if (!ok) return MVS_ERR_INVALID_ARGUMENT;
  if (geometry != MVS_OK) return geometry;
  if (batch_in_grid_z && batch > 65535) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int ls = launch();
  return ls != MVS_OK ? ls : lc.status();
}
}  // namespace

extern "C" {

int mvs_abi_version(void) { return MVS_ABI_VERSION; }

const char* mvs_status_string(int status) {
  switch (status) {
    case MVS_OK: return "ok";
    case MVS_ERR_INVALID_ARGUMENT: return "invalid argument";
    case MVS_ERR_UNSUPPORTED_VIEWS: return "n_views outside [1, MVS_MAX_VIEWS]";
    case MVS_ERR_TOO_LARGE: return "tensor exceeds the kernel's 32-bit index space";
    case MVS_ERR_HIP: return "HIP runtime error";
    default: return "unknown status";
  }
}

size_t mvs_sampling_workspace_bytes(int n_images, int d_count) {
  if (n_images <= 0 || d_count <= 0) return 0;
  return (size_t)n_images * (size_t)d_count * 9 * sizeof(float);
}

size_t mvs_cost_volume_workspace_bytes(int batch_size, int n_views, int channels, int h, int w,
                                       int d_count) {
  if (batch_size <= 0 || n_views <= 0 || channels <= 0 || h <= 0 || w <= 0 || d_count <= 0) return 0;
  return mvs::align256(mvs_sampling_workspace_bytes(batch_size * n_views, d_count)) +
         mvs::packed_bytes(batch_size, n_views, channels, h, w);
}

int mvs_plane_sampling(const float* K, const float* R, const float* T, const float* d_min,
                       const float* d_int, int batch_size, int n_views, int h, int w, int d_begin,
                       int d_count, float d_scale, float* sampling, void* stream) {
  if (!cams_ok(K, R, T, d_min, d_int) || !sampling) return MVS_ERR_INVALID_ARGUMENT;
  if (batch_size <= 0 || h < 2 || w < 2 || d_count <= 0 || d_begin < 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (n_views < 1 || n_views > MVS_MAX_VIEWS) return MVS_ERR_UNSUPPORTED_VIEWS;
  const mvs::LaunchCheck lc;
  mvs::launch_plane_sampling(K, R, T, d_min, d_int, batch_size, n_views, h, w, d_begin, d_count,
                             d_scale, sampling, (hipStream_t)stream);
  return lc.status();
}

int mvs_cost_volume_fwd_timed(const float* feat, const float* K, const float* R, const float* T,
                              const float* d_min, const float* d_int, int batch_size, int n_views,
                              int channels, int h, int w, int d_begin, int d_count, float d_scale,
                              float* workspace, float* cv_out, void* stream,
                              void* main_begin_event, void* main_end_event) {
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kF32, stream,
                              main_begin_event, main_end_event);
}

int mvs_cost_volume_fwd(const float* feat, const float* K, const float* R, const float* T,
                        const float* d_min, const float* d_int, int batch_size, int n_views,
                        int channels, int h, int w, int d_begin, int d_count, float d_scale,
                        float* workspace, float* cv_out, void* stream) {
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kF32, stream, nullptr,
                              nullptr);
}

int mvs_cost_volume_fwd_bf16(const float* feat, const float* K, const float* R, const float* T,
                             const float* d_min, const float* d_int, int batch_size, int n_views,
                             int channels, int h, int w, int d_begin, int d_count, float d_scale,
                             float* workspace, void* cv_out, void* stream) {
  if (n_views > 8) return MVS_ERR_UNSUPPORTED_VIEWS;
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kBf16, stream, nullptr,
                              nullptr);
}

int mvs_cost_volume_fwd_c4(const float* feat, const float* K, const float* R, const float* T,
                           const float* d_min, const float* d_int, int batch_size, int n_views,
                           int channels, int h, int w, int d_begin, int d_count, float d_scale,
                           float* workspace, float* cv_out, void* stream, void* main_begin_event,
                           void* main_end_event) {
  if (n_views > 8) return MVS_ERR_UNSUPPORTED_VIEWS;
  if ((uintptr_t)cv_out & 15u) return MVS_ERR_INVALID_ARGUMENT;
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kQuadF32, stream,
                              main_begin_event, main_end_event);
}

int mvs_cost_volume_fwd_c4_absmax(const float* feat, const float* K, const float* R, const float* T,
                                  const float* d_min, const float* d_int, int batch_size, int n_views,
                                  int channels, int h, int w, int d_begin, int d_count, float d_scale,
                                  float* workspace, float* cv_out, void* stream, void* main_begin_event,
                                  void* main_end_event, unsigned* feat_absmax) {
  if (n_views > 8) return MVS_ERR_UNSUPPORTED_VIEWS;
  if (((uintptr_t)cv_out & 15u) || !feat_absmax || ((uintptr_t)feat_absmax & 3u)) return MVS_ERR_INVALID_ARGUMENT;
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kQuadF32, stream,
                              main_begin_event, main_end_event, feat_absmax);
}

int mvs_cost_volume_fwd_c4_split(const float* feat, const float* K, const float* R, const float* T,
                                 const float* d_min, const float* d_int, int batch_size, int n_views,
                                 int channels, int h, int w, int d_begin, int d_count, float d_scale,
                                 float* workspace, void* cv_out, void* stream, void* main_begin_event,
                                 void* main_end_event, unsigned* feat_absmax) {
  if (n_views > 8) return MVS_ERR_UNSUPPORTED_VIEWS;
  if (((uintptr_t)cv_out & 15u) || !feat_absmax || ((uintptr_t)feat_absmax & 3u)) return MVS_ERR_INVALID_ARGUMENT;
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kQuadSplit, stream,
                              main_begin_event, main_end_event, feat_absmax);
}

int mvs_conv3d_split_weights(const float* weight, unsigned short* frag, int* weight_exp) {
  if (!weight || !frag || !weight_exp) return MVS_ERR_INVALID_ARGUMENT;
  int ew;
  if (!split_scale(weight, 8 * 32 * 27, &ew)) return MVS_ERR_INVALID_ARGUMENT;
  // frag[tap][lane][j]: lane (c = lane & 15, g = lane >> 4) holds B[k = 8g + j][col c] of the
  // 16x16x32 MFMA, column c < 8 = w_hi of output channel c, c >= 8 = w_lo of channel c - 8, k = input
  // channel; tap = (kz * 3 + ky) * 3 + kx; nn.Conv3d weight [8][32][3][3][3]
  for (int tap = 0; tap < 27; ++tap)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int c = lane & 15, ci = 8 * (lane >> 4) + j, co = c & 7;
        const SplitBits b = split_bits(std::ldexp(weight[(co * 32 + ci) * 27 + tap], ew));
        frag[(tap * 64 + lane) * 8 + j] = c < 8 ? b.hi : b.lo;
      }
  *weight_exp = ew;
  return MVS_OK;
}

int mvs_conv3d_s2_split_weights(const float* weight, unsigned short* frag, int* weight_exp) {
  if (!weight || !frag || !weight_exp) return MVS_ERR_INVALID_ARGUMENT;
  int ew;
  if (!split_scale(weight, 16 * 32 * 27, &ew)) return MVS_ERR_INVALID_ARGUMENT;
  // frag[tap][part][lane][j]: lane (c = lane & 15, g = lane >> 4) holds B[k = 8g + j][col c], column
  // c = output channel c, k = input channel; part 0 = hi, 1 = lo; nn.Conv3d weight [16][32][3][3][3]
  for (int tap = 0; tap < 27; ++tap)
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int co = lane & 15, ci = 8 * (lane >> 4) + j;
        const SplitBits b = split_bits(std::ldexp(weight[(co * 32 + ci) * 27 + tap], ew));
        frag[((tap * 2 + 0) * 64 + lane) * 8 + j] = b.hi;
        frag[((tap * 2 + 1) * 64 + lane) * 8 + j] = b.lo;
      }
  *weight_exp = ew;
  return MVS_OK;
}

int mvs_conv3d_s2_split_fwd(const void* x, int flags, const void* weight_frag, int weight_exp,
                            const unsigned* x_absmax, float* y, int batch, const int* dims,
                            const int* out_origin, const int* out_size, const int* pad, const float* bn_scale,
                            const float* bn_shift, const float* bn_mean, void* stream) {
  if (!x || !weight_frag || !y || !dims || !out_origin || !out_size || !pad || batch <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & ~MVS_CONV_IN_SPLIT) || ((flags & MVS_CONV_IN_SPLIT) && !x_absmax)) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)x & 15u) || ((uintptr_t)weight_frag & 15u) || ((uintptr_t)x_absmax & 3u))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  if (!exp_ok(weight_exp)) return MVS_ERR_INVALID_ARGUMENT;
  uint64_t vox = 1, ovox = 1;
  for (int d = 0; d < 3; ++d) {
    if (dims[d] <= 0 || out_size[d] <= 0 || out_origin[d] < 0 || pad[d] < 0) return MVS_ERR_INVALID_ARGUMENT;
    if (!s2_region_ok(out_origin[d], out_size[d], dims[d], pad[d])) return MVS_ERR_INVALID_ARGUMENT;
    vox *= (uint64_t)dims[d];
    ovox *= (uint64_t)out_size[d];
  }
  if (128ull * vox > 0xFFFFFFF0ull || (uint64_t)batch * ovox * 16ull >= (1ull << 40)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int st = mvs::launch_conv_s2_split(x, (flags & MVS_CONV_IN_SPLIT) != 0, weight_frag, weight_exp, x_absmax,
                                           y, batch, dims, out_origin, out_size, pad, bn_scale, bn_shift, bn_mean,
                                           (hipStream_t)stream);
  return st != MVS_OK ? st : lc.status();
}

int mvs_cost_volume_head_fwd(const float* feat, const float* K, const float* R, const float* T,
                             const float* d_min, const float* d_int, int batch_size, int n_views,
                             int channels, int h, int w, int d_begin, int d_count, float d_scale,
                             const void* w0_frag, int w0_exp, const float* bn0_scale, const float* bn0_shift,
                             const float* bn0_mean, const void* w1_frag, int w1_exp, const float* bn1_scale,
                             const float* bn1_shift, const float* bn1_mean, const int* pad,
                             const int* y1_origin, const int* y1_size, const int* scv_lo, const int* scv_hi,
                             float* workspace, unsigned* feat_absmax, float* y0, float* y1, void* scv,
                             void* stream, void* main_begin_event, void* main_end_event) {
  if (!feat || !workspace || !feat_absmax || !y0 || !y1 || !w0_frag || !w1_frag || !pad || !y1_origin ||
      !y1_size || !scv_lo || !scv_hi)
    return MVS_ERR_INVALID_ARGUMENT;
  if (!cams_ok(K, R, T, d_min, d_int) || d_begin < 0) return MVS_ERR_INVALID_ARGUMENT;
  if (n_views < 2 || n_views > 3) return MVS_ERR_UNSUPPORTED_VIEWS;
  if (channels != 32 || (d_count & 1)) return MVS_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)w0_frag) | ((uintptr_t)w1_frag) | ((uintptr_t)y0) | ((uintptr_t)scv)) & 15u) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)feat_absmax) & 3u) return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn0_scale, bn0_shift, bn0_mean) || !bn_all_or_none(bn1_scale, bn1_shift, bn1_mean))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!exp_ok(w0_exp) || !exp_ok(w1_exp)) return MVS_ERR_INVALID_ARGUMENT;
  Geometry g;
  int st = check_geometry(batch_size, n_views, channels, h, w, d_count, g, 16);
  if (st != MVS_OK) return st;
  const int n[3] = {d_count, h, w};
  uint64_t ovox = 1;
  for (int d = 0; d < 3; ++d) {
    if (pad[d] < 1 || !(pad[d] & 1)) return MVS_ERR_INVALID_ARGUMENT;
    if (y1_size[d] <= 0 || y1_origin[d] < 0 || !s2_region_ok(y1_origin[d], y1_size[d], n[d], pad[d]))
      return MVS_ERR_INVALID_ARGUMENT;
    if (scv_lo[d] < 0 || scv_hi[d] > n[d] || scv_lo[d] > scv_hi[d]) return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)y1_size[d];
  }
  if (128ull * (uint64_t)(scv_hi[0] - scv_lo[0]) * (uint64_t)(scv_hi[1] - scv_lo[1]) *
          (uint64_t)(scv_hi[2] - scv_lo[2]) > 0xFFFFFFF0ull ||
      (uint64_t)batch_size * ovox * 16ull >= (1ull << 40))
    return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  hipStream_t s = (hipStream_t)stream;
  const mvs::Cams cm{K, R, T, d_min, d_int, d_begin, d_scale};
  const float* bn0[3] = {bn0_scale, bn0_shift, bn0_mean};
  const float* bn1[3] = {bn1_scale, bn1_shift, bn1_mean};
  st = mvs::launch_cv_head(g, feat, cm, workspace, reinterpret_cast<uint32_t*>(feat_absmax), w0_frag, w0_exp, w1_frag,
                           w1_exp, bn0, bn1, y0, y1, scv, pad, y1_origin, y1_size, scv_lo, scv_hi, s,
                           (hipEvent_t)main_begin_event, (hipEvent_t)main_end_event);
  if (st != MVS_OK) return st;
  return lc.status();
}

int mvs_split_head_fwd(const void* scv, const unsigned* x_absmax, int batch, int d_count, int h, int w,
                       const void* w0_frag, int w0_exp, const float* bn0_scale, const float* bn0_shift,
                       const float* bn0_mean, const void* w1_frag, int w1_exp, const float* bn1_scale,
                       const float* bn1_shift, const float* bn1_mean, const int* pad, const int* y1_origin,
                       const int* y1_size, float* y0, float* y1, unsigned* y1_bound, void* stream,
                       void* main_begin_event, void* main_end_event) {
  if (!scv || !x_absmax || !y0 || !y1 || !w0_frag || !w1_frag || !pad || !y1_origin || !y1_size)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((uintptr_t)y1_bound & 3u) return MVS_ERR_INVALID_ARGUMENT;
  if (batch <= 0 || d_count <= 0 || h <= 0 || w <= 0 || (d_count & 1)) return MVS_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)scv) | ((uintptr_t)w0_frag) | ((uintptr_t)w1_frag) | ((uintptr_t)y0)) & 15u ||
      ((uintptr_t)x_absmax & 3u))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn0_scale, bn0_shift, bn0_mean) || !bn_all_or_none(bn1_scale, bn1_shift, bn1_mean))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!exp_ok(w0_exp) || !exp_ok(w1_exp)) return MVS_ERR_INVALID_ARGUMENT;
  const int n[3] = {d_count, h, w};
  uint64_t ovox = 1;
  for (int d = 0; d < 3; ++d) {
    if (pad[d] < 1 || !(pad[d] & 1)) return MVS_ERR_INVALID_ARGUMENT;
    if (y1_size[d] <= 0 || y1_origin[d] < 0 || !s2_region_ok(y1_origin[d], y1_size[d], n[d], pad[d]))
      return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)y1_size[d];
  }
  if (128ull * (uint64_t)d_count * (uint64_t)h * (uint64_t)w > 0xFFFFFFF0ull ||
      (uint64_t)batch * ovox * 16ull >= (1ull << 40))
    return MVS_ERR_TOO_LARGE;
  const Geometry g{batch, 2, 32, h, w, d_count, 0, 0};   // B, V, C, h, w, Dc, tiles, total
  const mvs::LaunchCheck lc;
  const float* bn0[3] = {bn0_scale, bn0_shift, bn0_mean};
  const float* bn1[3] = {bn1_scale, bn1_shift, bn1_mean};
  const int st = mvs::launch_split_head(g, scv, reinterpret_cast<const uint32_t*>(x_absmax), w0_frag, w0_exp, w1_frag,
                                        w1_exp, bn0, bn1, y0, y1, pad, y1_origin, y1_size,
                                        reinterpret_cast<uint32_t*>(y1_bound), (hipStream_t)stream,
                                        (hipEvent_t)main_begin_event, (hipEvent_t)main_end_event);
  return st != MVS_OK ? st : lc.status();
}

int mvs_conv3d_k3_split_fwd(const void* x, int flags, const void* weight_frag, int weight_exp,
                            const unsigned* x_absmax, float* y, int batch, int d, int h, int w,
                            const float* bn_scale, const float* bn_shift, const float* bn_mean, void* stream) {
  if (!x || !weight_frag || !y || batch <= 0 || d <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & ~MVS_CONV_IN_SPLIT) || ((flags & MVS_CONV_IN_SPLIT) && !x_absmax)) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)x & 15u) || ((uintptr_t)weight_frag & 15u) || ((uintptr_t)x_absmax & 3u))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  if (!exp_ok(weight_exp)) return MVS_ERR_INVALID_ARGUMENT;
  // one 32-bit buffer descriptor per sample volume (8 quads of 16 B per voxel) and 32-bit staging offsets
  if (128ull * (uint64_t)d * (uint64_t)h * (uint64_t)w > 0xFFFFFFF0ull) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int st = mvs::launch_conv3d_split(x, (flags & MVS_CONV_IN_SPLIT) != 0, weight_frag, weight_exp, x_absmax,
                                          y, batch, d, h, w, bn_scale, bn_shift, bn_mean, (hipStream_t)stream);
  return st != MVS_OK ? st : lc.status();
}

int mvs_cost_volume_fwd_c4_bf16(const float* feat, const float* K, const float* R, const float* T,
                                const float* d_min, const float* d_int, int batch_size, int n_views,
                                int channels, int h, int w, int d_begin, int d_count, float d_scale,
                                float* workspace, void* cv_out, void* stream, void* main_begin_event,
                                void* main_end_event) {
  if (n_views > 8) return MVS_ERR_UNSUPPORTED_VIEWS;
  if ((uintptr_t)cv_out & 7u) return MVS_ERR_INVALID_ARGUMENT;
  return cost_volume_fwd_impl(feat, K, R, T, d_min, d_int, batch_size, n_views, channels, h, w,
                              d_begin, d_count, d_scale, workspace, cv_out, CvStore::kQuadBf16, stream,
                              main_begin_event, main_end_event);
}

int mvs_homography_warp_fwd(const float* feat, const float* K, const float* R, const float* T,
                            const float* d_min, const float* d_int, int batch_size, int n_views,
                            int channels, int h, int w, int d_begin, int d_count, float d_scale,
                            float* workspace, float* warped_out, void* stream) {
  if (!feat || !workspace || !warped_out) return MVS_ERR_INVALID_ARGUMENT;
  Geometry g;
  int st = check_geometry(batch_size, n_views, channels, h, w, d_count, g);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  st = mvs_plane_sampling(K, R, T, d_min, d_int, batch_size, n_views, h, w, d_begin, d_count,
                          d_scale, workspace, stream);
  if (st != MVS_OK) return st;
  mvs::launch_warp(g, feat, workspace, warped_out, (hipStream_t)stream);
  return lc.status();
}

int mvs_assemble_cost_volume_fwd(const float* warped, int batch_size, int n_views, int channels,
                                 int d, int h, int w, float* cv_out, void* stream) {
  if (!warped || !cv_out || batch_size <= 0 || channels <= 0 || d <= 0 || h <= 0 || w <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (n_views < 1) return MVS_ERR_UNSUPPORTED_VIEWS;
  const mvs::LaunchCheck lc;
  mvs::launch_variance(warped, batch_size, n_views, (size_t)channels * d * h * w, cv_out,
                       (hipStream_t)stream);
  return lc.status();
}

size_t mvs_cost_volume_bwd_workspace_bytes(int batch_size, int n_views, int channels, int h, int w,
                                           int d_count, int flags) {
  if (batch_size <= 0 || n_views <= 0 || channels <= 0 || h <= 0 || w <= 0 || d_count <= 0) return 0;
  if (flags & ~MVS_BWD_DETERMINISTIC) return 0;
  return mvs::cost_volume_bwd_workspace_bytes(batch_size, n_views, channels, h, w, d_count,
                                              (flags & MVS_BWD_DETERMINISTIC) != 0);
}

int mvs_cost_volume_bwd(const float* feat, const float* workspace, const float* grad_cv,
                        int batch_size, int n_views, int channels, int h, int w, int d_count,
                        int flags, void* bwd_workspace, float* grad_feat, void* stream) {
  if (!feat || !workspace || !grad_cv || !grad_feat || (n_views > 1 && !bwd_workspace))
    return MVS_ERR_INVALID_ARGUMENT;
  if (flags & ~MVS_BWD_DETERMINISTIC) return MVS_ERR_INVALID_ARGUMENT;
  Geometry g;
  const int st = check_geometry(batch_size, n_views, channels, h, w, d_count, g);
  if (st != MVS_OK) return st;
  // the packed backward reads grad_cv through a 32-bit descriptor over one 4-channel chunk
  if (n_views >= 2 && n_views <= 8 && 16ull * (uint64_t)d_count * (uint64_t)h * (uint64_t)w >= (1ull << 31))
    return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int ls = mvs::launch_cost_volume_bwd(g, feat, workspace, grad_cv, bwd_workspace, grad_feat,
                                             (flags & MVS_BWD_DETERMINISTIC) != 0, (hipStream_t)stream);
  return ls != MVS_OK ? ls : lc.status();
}

int mvs_extract_depth_map_fwd(const float* prob, const float* d_batch, int batch_size, int d,
                              int h, int w, int n_est, float* depth_out, void* stream) {
  if (!prob || !d_batch || !depth_out || batch_size <= 0 || d <= 0 || h <= 0 || w <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (n_est < 1) return MVS_ERR_INVALID_ARGUMENT;
  if (n_est > d) n_est = d;  // every plane index is < n_est: all planes kept
  if (n_est > 16) return MVS_ERR_INVALID_ARGUMENT;
  const mvs::LaunchCheck lc;
  mvs::launch_soft_argmin(prob, d_batch, batch_size, d, (uint32_t)h * (uint32_t)w, n_est, depth_out,
                          (hipStream_t)stream);
  return lc.status();
}

int mvs_normalize_images(const unsigned char* rgb, int n_images, int h, int w, const float* mean,
                         const float* std_dev, float* out, void* stream) {
  if (!rgb || !out || !mean || !std_dev || n_images <= 0 || h <= 0 || w <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)rgb & 3u) || ((uintptr_t)out & 15u)) return MVS_ERR_INVALID_ARGUMENT;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  if (hw >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  for (int c = 0; c < 3; ++c)
    if (!(std_dev[c] != 0.0f)) return MVS_ERR_INVALID_ARGUMENT;
  const mvs::LaunchCheck lc;
  mvs::launch_normalize_images(rgb, n_images, (uint32_t)hw, mean, std_dev, out, (hipStream_t)stream);
  return lc.status();
}

int mvs_depth_threshold(const float* depth, size_t n, float lo, float hi, float* out, void* stream) {
  if (!depth || !out) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)depth & 15u) || ((uintptr_t)out & 15u)) return MVS_ERR_INVALID_ARGUMENT;
  if (n == 0) return MVS_OK;
  const mvs::LaunchCheck lc;
  mvs::launch_depth_threshold(depth, n, lo, hi, out, (hipStream_t)stream);
  return lc.status();
}

int mvs_conv2d_fwd(const float* x, const float* weight, float* y, int n, int c_in, int c_out, int h, int w,
                   int k, int stride, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                   unsigned* y_bound, void* stream) {
  if (!x || !weight || !y || n <= 0 || n > 65535 || h <= 0 || w <= 0 || stride <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  // staging offsets inside one image are 32-bit
  if ((uint64_t)c_in * (uint64_t)h * (uint64_t)w >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int st = mvs::launch_conv2d_narrow(x, weight, y, n, c_in, c_out, h, w, k, stride, bn_scale, bn_shift,
                                           bn_mean, y_bound, (hipStream_t)stream);
  return st != MVS_OK ? st : lc.status();
}

int mvs_conv2d_split_weights(const float* weight, int c_in, int c_out, int k, unsigned short* frag, int* weight_exp) {
  if (!weight || !frag || !weight_exp || k <= 0 || k > 7) return MVS_ERR_INVALID_ARGUMENT;
  if (!(c_in == 8 || c_in == 16 || c_in == 32) || !(c_out == 8 || (c_out > 0 && c_out % 16 == 0)))
    return MVS_ERR_INVALID_ARGUMENT;
  const int taps = k * k;
  int ew;
  if (!split_scale(weight, (size_t)c_out * c_in * taps, &ew)) return MVS_ERR_INVALID_ARGUMENT;
  const int kbs = mvs::conv2d_split_kblocks(c_in, k), tpb = 32 / c_in, cpt = c_in / 8;
  const bool narrow = c_out == 8;
  const int nbs = narrow ? 1 : c_out / 16;
  auto split = [&](int co, int ci, int t) {   // taps past k * k pad the last K block with zeros
    return split_bits(t < taps ? std::ldexp(weight[((size_t)co * c_in + ci) * taps + t], ew) : 0.0f);
  };
  for (int kb = 0; kb < kbs; ++kb)
    for (int nb = 0; nb < nbs; ++nb)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int c = lane & 15, g = lane >> 4;
          const int t = kb * tpb + g / cpt, ci = 8 * (g % cpt) + j;
          const SplitBits b = split(narrow ? c & 7 : nb * 16 + c, ci, t);
          if (narrow) {   // columns 0..7 hi, 8..15 lo of the 8 output channels
            frag[((size_t)kb * 64 + lane) * 8 + j] = c < 8 ? b.hi : b.lo;
          } else {
            const size_t base = ((((size_t)kb * nbs + nb) * 2) * 64 + lane) * 8 + j;
            frag[base] = b.hi;
            frag[base + 64 * 8] = b.lo;
          }
        }
  *weight_exp = ew;
  return MVS_OK;
}

int mvs_conv2d_split_fwd(const float* x, const void* weight_frag, int weight_exp, float* y, int n, int c_in,
                         int c_out, int h, int w, int k, int stride, const float* bn_scale, const float* bn_shift,
                         const float* bn_mean, const unsigned* x_bound, unsigned* y_bound, void* stream) {
  if (!x || !weight_frag || !y || !x_bound || n <= 0 || n > 65535 || h <= 0 || w <= 0 || stride <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(weight_frag) % 16) return MVS_ERR_INVALID_ARGUMENT;
  // one image's buffer resource and staging offsets are 32-bit
  if ((uint64_t)c_in * (uint64_t)h * (uint64_t)w * 4u >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int st = mvs::launch_conv2d_split(x, weight_frag, weight_exp, y, n, c_in, c_out, h, w, k, stride, bn_scale,
                                          bn_shift, bn_mean, x_bound, y_bound, (hipStream_t)stream);
  return st != MVS_OK ? st : lc.status();
}

int mvs_conv3d_k3_fwd(const float* x, int flags, const float* weight, float* y, int batch, int c_in,
                      int c_out, int d, int h, int w, const float* bn_scale, const float* bn_shift,
                      const float* bn_mean, const float* x2, const float* in_bn, void* stream) {
  if (in_bn && (c_out != 1 || flags || !x2 || bn_scale)) return MVS_ERR_INVALID_ARGUMENT;
  if (!in_bn && x2) return MVS_ERR_INVALID_ARGUMENT;
  if (!x || !weight || !y || batch <= 0 || c_in <= 0 || d <= 0 || h <= 0 || w <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (c_out != 1 && c_out != 8) return MVS_ERR_INVALID_ARGUMENT;
  if (flags & ~(MVS_CONV_IN_C4 | MVS_CONV_WINO_Z | MVS_CONV_IN_BF16)) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_IN_BF16) && (!(flags & MVS_CONV_IN_C4) || ((uintptr_t)x & 7u))) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_WINO_Z) && c_out != 8) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_IN_C4) && (c_in % 4 || (!(flags & MVS_CONV_IN_BF16) && ((uintptr_t)x & 15u))))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  // staging offsets inside one channel volume are 32-bit
  if ((uint64_t)d * (uint64_t)h * (uint64_t)w >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int quads = (flags & MVS_CONV_IN_C4) ? ((flags & MVS_CONV_IN_BF16) ? 2 : 1) : 0;
  mvs::launch_conv3d_k3_narrow(x, quads, (flags & MVS_CONV_WINO_Z) != 0, weight, y, batch,
                               c_in, c_out, d, h, w,
                               bn_scale, bn_shift, bn_mean,
                               (hipStream_t)stream, x2, in_bn);
  return lc.status();
}

size_t mvs_conv3d_k3_wgrad_workspace_bytes(int batch, int c_in, int d, int h, int w) {
  if (batch <= 0 || c_in <= 0 || d <= 0 || h <= 0 || w <= 0) return 0;
  return mvs::conv3d_wgrad_workspace_bytes(batch, c_in, d, h, w);
}

int mvs_conv3d_k3_wgrad(const float* x, const float* gy, int batch, int c_in, int c_out, int d, int h, int w,
                        float* dw, void* workspace, void* stream) {
  if (!x || !gy || !dw || !workspace || batch <= 0 || d <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (!mvs::conv3d_wgrad_supported(c_in, c_out)) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)d * (uint64_t)h * (uint64_t)w >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_conv3d_wgrad(x, gy, batch, c_in, c_out, d, h, w, static_cast<float*>(workspace), dw,
                           (hipStream_t)stream);
  return lc.status();
}

// ---- training extension (include/train/mvs_region_train.h) ----
int mvs_train_abi_version(void) { return MVS_TRAIN_ABI_VERSION; }

size_t mvs_conv3d_region_wgrad_workspace_bytes(int batch, int channels, const int* in_size) {
  if (region_wgrad_geometry(batch, channels, in_size) != MVS_OK) return 0;
  return mvs::conv3d_region_wgrad_workspace_bytes(batch, channels, in_size);
}

int mvs_conv3d_region_wgrad(const float* x, const float* gy, int batch, int channels, const int* in_size,
                            float* dw, float* workspace, void* stream) {
  return train_launch(aligned16(x, gy, dw, workspace), region_wgrad_geometry(batch, channels, in_size), false, batch,
                      [&] {
                        mvs::launch_conv3d_region_wgrad(x, gy, batch, channels, in_size, workspace, dw,
                                                        (hipStream_t)stream);
                        return MVS_OK;
                      });
}

size_t mvs_conv3d_s2_region_wgrad_workspace_bytes(int batch, const int* dims, const int* out_size) {
  if (s2_region_bwd_geometry(batch, dims, nullptr, out_size) != MVS_OK) return 0;
  return mvs::conv3d_s2_wgrad_workspace_bytes(batch, dims, out_size);
}

int mvs_conv3d_s2_region_wgrad(const float* x, const float* gy, int batch, const int* dims, const int* pad_lo,
                               const int* out_size, float* dw, float* workspace, void* stream) {
  return train_launch(aligned16(x, gy, dw, workspace) && pad_lo, s2_region_bwd_geometry(batch, dims, pad_lo, out_size),
                      false, batch, [&] {
                        mvs::launch_conv3d_s2_wgrad(x, gy, batch, dims, pad_lo, out_size, workspace, dw,
                                                    (hipStream_t)stream);
                        return MVS_OK;
                      });
}

int mvs_conv3d_s2_region_dgrad(const float* gy, const float* w27, int batch, const int* dims, const int* pad_lo,
                               const int* out_size, float* gx, void* stream) {
  return train_launch(aligned16(gy, w27, gx) && pad_lo, s2_region_bwd_geometry(batch, dims, pad_lo, out_size), true,
                      batch, [&] {
                        mvs::launch_conv3d_s2_dgrad(gy, w27, gx, batch, dims, pad_lo, out_size, (hipStream_t)stream);
                        return MVS_OK;
                      });
}

size_t mvs_conv3d_t2_region_wgrad_workspace_bytes(int batch, int c_in, int c_out, const int* in_size,
                                                  const int* out_size) {
  if (t2_region_bwd_geometry(batch, c_in, c_out, in_size, nullptr, out_size) != MVS_OK) return 0;
  return mvs::conv3d_t2_wgrad_workspace_bytes(batch, c_in, c_out, in_size, out_size);
}

int mvs_conv3d_t2_region_wgrad(const float* x, const float* gy, int batch, int c_in, int c_out, const int* in_size,
                               const int* crop, const int* out_size, float* dw, float* workspace, void* stream) {
  return train_launch(aligned16(x, gy, dw, workspace) && crop,
                      t2_region_bwd_geometry(batch, c_in, c_out, in_size, crop, out_size), false, batch, [&] {
                        mvs::launch_conv3d_t2_wgrad(x, gy, batch, c_in, c_out, in_size, crop, out_size, workspace, dw,
                                                    (hipStream_t)stream);
                        return MVS_OK;
                      });
}

int mvs_conv3d_t2_region_dgrad(const float* gy, const float* w27, int batch, int c_in, int c_out, const int* in_size,
                               const int* crop, const int* out_size, float* gx, void* stream) {
  return train_launch(aligned16(gy, w27, gx) && crop,
                      t2_region_bwd_geometry(batch, c_in, c_out, in_size, crop, out_size), true, batch, [&] {
                        return mvs::launch_conv3d_t2_dgrad(gy, w27, gx, batch, c_in, c_out, in_size, crop, out_size,
                                                           (hipStream_t)stream);
                      });
}

size_t mvs_deconv3d_k3s2_wgrad_workspace_bytes(int batch, int c_in, int c_out, const int* in_size,
                                               const int* out_size) {
  if (deconv3d_bwd_geometry(batch, c_in, c_out, in_size, nullptr, out_size) != MVS_OK) return 0;
  return mvs::deconv3d_wgrad_workspace_bytes(batch, in_size, out_size);
}

int mvs_deconv3d_k3s2_wgrad(const float* x, int flags, const float* gy, int batch, int c_in, int c_out,
                            const int* in_size, const int* crop, const int* out_size, float* dw, float* workspace,
                            void* stream) {
  return train_launch(aligned16(x, gy, dw, workspace) && crop && !(flags & ~MVS_LAYOUT_CHANNELS_LAST),
                      deconv3d_bwd_geometry(batch, c_in, c_out, in_size, crop, out_size), false, batch, [&] {
                        mvs::launch_deconv3d_wgrad(x, (flags & MVS_LAYOUT_CHANNELS_LAST) != 0, gy, batch, in_size, crop,
                                                   out_size, workspace, dw, (hipStream_t)stream);
                        return MVS_OK;
                      });
}

int mvs_deconv3d_k3s2_dgrad(const float* gy, const float* w27, int flags, int batch, int c_in, int c_out,
                            const int* in_size, const int* crop, const int* out_size, float* gx, void* stream) {
  return train_launch(aligned16(gy, w27, gx) && crop && !(flags & ~MVS_LAYOUT_CHANNELS_LAST),
                      deconv3d_bwd_geometry(batch, c_in, c_out, in_size, crop, out_size), false, batch, [&] {
                        mvs::launch_deconv3d_dgrad(gy, w27, gx, (flags & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, in_size,
                                                   crop, out_size, (hipStream_t)stream);
                        return MVS_OK;
                      });
}

int mvs_conv2d_wgrad_plan(int n, int c_in, int c_out, int h, int w, int k, int stride, int* tiles, int* slots) {
  const int g = conv2d_bwd_geometry(n, c_in, c_out, h, w, k, stride);
  if (g != MVS_OK) return g;
  const mvs::Conv2dWgradPlan p = mvs::conv2d_wgrad_plan(n, c_in, c_out, h, w, k, stride);
  if (tiles) *tiles = p.tiles;
  if (slots) *slots = p.slots;
  return MVS_OK;
}

size_t mvs_conv2d_wgrad_workspace_bytes(int n, int c_in, int c_out, int h, int w, int k, int stride) {
  if (conv2d_bwd_geometry(n, c_in, c_out, h, w, k, stride) != MVS_OK) return 0;
  const mvs::Conv2dWgradPlan p = mvs::conv2d_wgrad_plan(n, c_in, c_out, h, w, k, stride);
  return (size_t)p.slots * p.slot_floats * sizeof(float);
}

int mvs_conv2d_wgrad(const float* x, const float* gy, int n, int c_in, int c_out, int h, int w, int k, int stride,
                     float* dw, float* workspace, void* stream) {
  return train_launch(aligned16(x, gy, dw, workspace), conv2d_bwd_geometry(n, c_in, c_out, h, w, k, stride), false, n,
                      [&] {
                        return mvs::launch_conv2d_wgrad(x, gy, n, c_in, c_out, h, w, k, stride, workspace, dw,
                                                        (hipStream_t)stream);
                      });
}

int mvs_conv2d_dgrad(const float* gy, const float* weight, int n, int c_in, int c_out, int h, int w, int k,
                     int stride, float* gx, void* stream) {
  return train_launch(aligned16(gy, weight, gx), conv2d_bwd_geometry(n, c_in, c_out, h, w, k, stride), true, n, [&] {
    return mvs::launch_conv2d_dgrad(gy, weight, gx, n, c_in, c_out, h, w, k, stride, (hipStream_t)stream);
  });
}

int mvs_conv_head_fp32_fwd(const float* cv4, int batch, int d, int h, int w, const float* w0_wz,
                           const float* bn0_scale, const float* bn0_shift, const float* bn0_mean, const float* w1,
                           const float* w1_pass, const float* bn1_scale, const float* bn1_shift,
                           const float* bn1_mean, const int* pad, const int* y1_origin, const int* y1_size,
                           float* y0, float* y1, void* stream, void* ev0, void* ev1) {
  if (!cv4 || !w0_wz || !w1 || !w1_pass || !y0 || !y1 || !pad || !y1_origin || !y1_size || batch <= 0 || d <= 0 ||
      h <= 0 || w <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)cv4 | (uintptr_t)w1 | (uintptr_t)w1_pass) & 15u) return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn0_scale, bn0_shift, bn0_mean) || !bn_all_or_none(bn1_scale, bn1_shift, bn1_mean))
    return MVS_ERR_INVALID_ARGUMENT;
  const int n[3] = {d, h, w};
  uint64_t ovox = (uint64_t)batch;
  for (int k = 0; k < 3; ++k) {
    if (pad[k] < 1 || !(pad[k] & 1)) return MVS_ERR_INVALID_ARGUMENT;   // the fused windows need P odd
    if (y1_size[k] <= 0 || y1_origin[k] < 0 || y1_origin[k] + y1_size[k] > n[k]) return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)y1_size[k];
  }
  if ((uint64_t)d * h * w >= (1ull << 31) || ovox >= (1ull << 31) || (uint64_t)d * h * w * 64u >= 0xFFFFFFC0ull)
    return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_conv_head_fp32(cv4, batch, d, h, w, w0_wz, bn0_scale, bn0_shift, bn0_mean, w1, w1_pass, bn1_scale,
                             bn1_shift, bn1_mean, pad, y1_origin, y1_size, y0, y1, (hipStream_t)stream,
                             (hipEvent_t)ev0, (hipEvent_t)ev1);
  return lc.status();
}

int mvs_deconv3d_k3s2_fwd(const float* x, const float* x2, int flags, int batch, int c_in, int c_out,
                          int rd, int rh, int rw, int x0d, int x0h, int x0w, const float* weight, int d,
                          int h, int w, int pd, int ph, int pw, const float* bn_scale,
                          const float* bn_shift, const float* bn_mean, const float* residual, float* y,
                          void* stream) {
  if (!x || !weight || !y || batch <= 0 || c_in <= 0 || c_in > 64 || c_out != 8) return MVS_ERR_INVALID_ARGUMENT;
  if (flags & ~(MVS_LAYOUT_CHANNELS_LAST | MVS_DECONV_WEIGHT_TAPS)) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_LAYOUT_CHANNELS_LAST) && (c_in % 4 || ((uintptr_t)x & 15u) || ((uintptr_t)x2 & 15u)))
    return MVS_ERR_INVALID_ARGUMENT;   // 16-byte channel-quad loads
  if (rd <= 0 || rh <= 0 || rw <= 0 || d <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (x0d < 0 || x0h < 0 || x0w < 0 || pd < 0 || ph < 0 || pw < 0) return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  // the region input is read through 32-bit buffer descriptors over the whole batch
  if ((uint64_t)batch * c_in * rd * rh * rw * 4u >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  const int layout = (flags & MVS_LAYOUT_CHANNELS_LAST) ? ((flags & MVS_DECONV_WEIGHT_TAPS) ? 3 : 1)
                                                        : ((flags & MVS_DECONV_WEIGHT_TAPS) ? 2 : 0);
  const mvs::LaunchCheck lc;
  mvs::launch_deconv3d_k3s2(x, x2, layout, batch, c_in, rd, rh, rw, x0d, x0h,
                            x0w, weight, d, h, w, pd, ph, pw, bn_scale, bn_shift, bn_mean, residual, y,
                            (hipStream_t)stream);
  return lc.status();
}

int mvs_conv3d_region_fwd(int mode, int flags, const float* x, const float* x2, const float* weight, float* y,
                          int batch, int c_in, int c_out, const int* dims, const int* out_origin,
                          const int* out_size, const int* in_origin, const int* in_size,
                          const int* pad, const float* bn_scale, const float* bn_shift,
                          const float* bn_mean, const unsigned* x_absmax, unsigned* y_bound, void* stream) {
  if (!x || !weight || !y || !dims || !out_origin || !out_size || batch <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((uintptr_t)y_bound & 3u) return MVS_ERR_INVALID_ARGUMENT;
  if (mode < MVS_CONV_S1 || mode > MVS_CONV_T2 ||
      (flags & ~(MVS_CONV_OUT_NCDHW | MVS_CONV_IN_C4 | MVS_CONV_IN_BF16 | MVS_CONV_IN_SPLIT | MVS_CONV_PER_LANE |
                 MVS_CONV_S2_LDS)))
    return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_S2_LDS) && (flags & MVS_CONV_PER_LANE)) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_IN_BF16) && !(flags & MVS_CONV_IN_C4)) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_IN_SPLIT) && (!(flags & MVS_CONV_IN_C4) || (flags & MVS_CONV_IN_BF16) || !x_absmax ||
                                      ((uintptr_t)x_absmax & 3u)))
    return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_IN_C4) && (mode != MVS_CONV_S2 || c_in % 4)) return MVS_ERR_INVALID_ARGUMENT;
  if (mode != MVS_CONV_S2 && (!in_origin || !in_size)) return MVS_ERR_INVALID_ARGUMENT;
  if (!both_or_neither(in_origin, in_size)) return MVS_ERR_INVALID_ARGUMENT;
  const bool boxed = in_origin != nullptr;   // S2: x holds the box [in_origin, + in_size) of the volume
  if (mode != MVS_CONV_S1 && !pad) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)x | (uintptr_t)x2 | (uintptr_t)weight) & 15u) return MVS_ERR_INVALID_ARGUMENT;   // 16-byte loads
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  uint64_t ovox = (uint64_t)batch, ivox = (uint64_t)batch, nvox = (uint64_t)batch * c_in;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] <= 0 || out_size[k] <= 0 || out_origin[k] < 0 || out_origin[k] + out_size[k] > dims[k])
      return MVS_ERR_INVALID_ARGUMENT;
    if (boxed && (in_size[k] <= 0 || in_origin[k] < 0 || in_origin[k] + in_size[k] > dims[k]))
      return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)out_size[k];
    ivox *= (uint64_t)(boxed ? in_size[k] : dims[k]);
    nvox *= (uint64_t)dims[k];
  }
  // 32-bit row indices; per sample, 32-bit buffer descriptors over the input (S2: the 16 channel planes
  // or 4 channel quads of one 16-channel block, 64 B per voxel; S1 / T2: the region tensor)
  uint64_t svox = 1;
  for (int k = 0; k < 3; ++k) svox *= (uint64_t)(boxed ? in_size[k] : dims[k]);
  const uint64_t desc_bytes = mode == MVS_CONV_S2 ? svox * 64u : svox * (uint64_t)c_in * 4u;
  if (ovox >= (1ull << 31) || desc_bytes >= 0xFFFFFFC0ull || ivox * (uint64_t)c_in >= (1ull << 62) ||
      nvox >= (1ull << 62))
    return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int quads = (flags & MVS_CONV_IN_C4)
                        ? ((flags & MVS_CONV_IN_SPLIT) ? 3 : ((flags & MVS_CONV_IN_BF16) ? 2 : 1)) : 0;
  const int st = mvs::launch_conv3d_region(mode, (flags & MVS_CONV_OUT_NCDHW) != 0, quads,
                                           x, x2, weight, y, batch, c_in, c_out, dims, out_origin, out_size,
                                           in_origin, in_size, pad, bn_scale, bn_shift, bn_mean,
                                           (hipStream_t)stream, reinterpret_cast<const uint32_t*>(x_absmax),
                                           reinterpret_cast<uint32_t*>(y_bound), (flags & MVS_CONV_PER_LANE) != 0,
                                           nullptr, nullptr, (flags & MVS_CONV_S2_LDS) != 0);
  if (st != MVS_OK) return st;
  return lc.status();
}

int mvs_conv3d_s2_cells_geometry(int c_in, int c_out, const int* out_size, long long* geometry) {
  if (!out_size || !geometry || c_in <= 0 || c_out <= 0) return MVS_ERR_INVALID_ARGUMENT;
  uint64_t ovox = 1;
  for (int k = 0; k < 3; ++k) {
    if (out_size[k] <= 0) return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)out_size[k];
  }
  if (ovox >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  return mvs::conv3d_s2_cells_geometry(c_in, c_out, out_size, geometry);
}

int mvs_conv3d_region_split_weights(const float* weight, int c_in, int c_out, unsigned short* frag, int* weight_exp) {
  if (!weight || !frag || !weight_exp) return MVS_ERR_INVALID_ARGUMENT;
  if (c_out <= 0 || c_out % 16 || !(c_in == 16 || (c_in > 0 && c_in % 32 == 0))) return MVS_ERR_INVALID_ARGUMENT;
  int ew;
  if (!split_scale(weight, (size_t)27 * c_out * c_in, &ew)) return MVS_ERR_INVALID_ARGUMENT;
  // frag[kb][nb][part][lane][j]: lane (c = lane & 15, g = lane >> 4) holds B[k = 8g + j][column c] of the
  // 16x16x32 MFMA for output channel nb * 16 + c; part 0 = fp16(w 2^ew), 1 = fp16(w 2^ew - part 0).
  // K block kb: c_in >= 32: tap kb / (c_in / 32), input channel (kb % (c_in / 32)) * 32 + 8g + j;
  // c_in = 16: tap 2 kb + (g >> 1) (zero past tap 26), input channel 8 (g & 1) + j.  weight [27][c_out][c_in]
  const int kbs = mvs::conv3d_region_split_kblocks(c_in), nbs = c_out / 16;
  for (int kb = 0; kb < kbs; ++kb)
    for (int nb = 0; nb < nbs; ++nb)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int c = lane & 15, gq = lane >> 4, co = nb * 16 + c;
          int tap, ci;
          if (c_in == 16) {
            tap = 2 * kb + (gq >> 1);
            ci = 8 * (gq & 1) + j;
          } else {
            tap = kb / (c_in / 32);
            ci = (kb % (c_in / 32)) * 32 + 8 * gq + j;
          }
          const SplitBits b =
              split_bits(tap < 27 ? std::ldexp(weight[((size_t)tap * c_out + co) * c_in + ci], ew) : 0.0f);
          const size_t base = ((((size_t)kb * nbs + nb) * 2) * 64 + lane) * 8 + j;
          frag[base] = b.hi;
          frag[base + 64 * 8] = b.lo;
        }
  *weight_exp = ew;
  return MVS_OK;
}

int mvs_conv3d_region_split_fwd(int mode, int flags, const float* x, const float* x2, const void* weight_frag,
                                int weight_exp, float* y, int batch, int c_in, int c_out, const int* dims,
                                const int* out_origin, const int* out_size, const int* in_origin, const int* in_size,
                                const int* pad, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                const unsigned* x_bound, const unsigned* x2_bound, unsigned* y_bound,
                                const float* y_addend, const int* store_origin, const int* store_size, double* stats,
                                float* y_mid, float* y_high, const float* in_bn, void* stream) {
  if (!x || !weight_frag || !y || !dims || !out_origin || !out_size || batch <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (!both_or_neither(store_origin, store_size) || ((uintptr_t)stats & 7u) || ((uintptr_t)in_bn & 15u))
    return MVS_ERR_INVALID_ARGUMENT;
  if (store_origin)   // the store box lies inside the output region
    for (int k = 0; k < 3; ++k)
      if (store_size[k] <= 0 || store_origin[k] < out_origin[k] ||
          store_origin[k] + store_size[k] > out_origin[k] + out_size[k])
        return MVS_ERR_INVALID_ARGUMENT;
  if (mode < MVS_CONV_S1 || mode > MVS_CONV_T2 ||
      (flags & ~(MVS_CONV_OUT_NCDHW | MVS_CONV_IN_C4 | MVS_CONV_IN_SPLIT | MVS_CONV_PER_LANE | MVS_CONV_T2_LDS)))
    return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_T2_LDS) && mode != MVS_CONV_T2) return MVS_ERR_INVALID_ARGUMENT;
  // S2 reads the split cost volume (its 8 bound words in x_bound), S1 / T2 an fp32 region tensor
  const bool s2 = mode == MVS_CONV_S2;
  const int in_flags = MVS_CONV_IN_C4 | MVS_CONV_IN_SPLIT;
  if (s2 != ((flags & in_flags) == in_flags) || (!s2 && (flags & in_flags))) return MVS_ERR_INVALID_ARGUMENT;
  if (s2 && (x2 || !x_bound || c_in != 32)) return MVS_ERR_INVALID_ARGUMENT;
  if (!both_or_neither(in_origin, in_size) || (!s2 && !in_origin)) return MVS_ERR_INVALID_ARGUMENT;
  if (mode != MVS_CONV_S1 && !pad) return MVS_ERR_INVALID_ARGUMENT;
  int io[3] = {0, 0, 0}, is[3] = {dims[0], dims[1], dims[2]};   // S2 without a box: the whole volume
  if (in_origin)
    for (int k = 0; k < 3; ++k) {
      io[k] = in_origin[k];
      is[k] = in_size[k];
    }
  // every mode scales its input by the bound words (S2: the split volume's; S1 / T2: the region
  // tensor's, raised by the kernel that wrote it): without them the fp16 hi parts could overflow
  if (!x_bound || (x2 && !x2_bound)) return MVS_ERR_INVALID_ARGUMENT;   // a sum needs both bounds
  if (((uintptr_t)x | (uintptr_t)x2 | (uintptr_t)weight_frag) & 15u ||
      ((uintptr_t)x_bound | (uintptr_t)x2_bound | (uintptr_t)y_bound) & 3u)
    return MVS_ERR_INVALID_ARGUMENT;
  if (!exp_ok(weight_exp)) return MVS_ERR_INVALID_ARGUMENT;
  if (!bn_all_or_none(bn_scale, bn_shift, bn_mean)) return MVS_ERR_INVALID_ARGUMENT;
  uint64_t ovox = (uint64_t)batch, svox = 1;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] <= 0 || out_size[k] <= 0 || out_origin[k] < 0 || out_origin[k] + out_size[k] > dims[k])
      return MVS_ERR_INVALID_ARGUMENT;
    if (is[k] <= 0 || io[k] < 0 || io[k] + is[k] > dims[k]) return MVS_ERR_INVALID_ARGUMENT;
    ovox *= (uint64_t)out_size[k];
    svox *= (uint64_t)is[k];
  }
  if (ovox >= (1ull << 31) || svox * (uint64_t)c_in * 4u >= 0xFFFFFFC0ull) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  const int st = mvs::launch_conv3d_region_split(
      mode, (flags & MVS_CONV_OUT_NCDHW) != 0, x, x2, weight_frag, weight_exp, y, batch, c_in, c_out, dims, out_origin,
      out_size, io, is, pad, bn_scale, bn_shift, bn_mean, reinterpret_cast<const uint32_t*>(x_bound),
      reinterpret_cast<const uint32_t*>(x2_bound), reinterpret_cast<uint32_t*>(y_bound), (hipStream_t)stream,
      (flags & MVS_CONV_PER_LANE) != 0, y_addend, store_origin, store_size, stats, y_mid, y_high, in_bn,
      (flags & MVS_CONV_T2_LDS) != 0);
  if (st != MVS_OK) return st;
  return lc.status();
}

long long mvs_conv3d_region_split_stats_slots(int mode, int flags, int batch, int c_in, int c_out,
                                              const int* out_size) {
  if (!out_size || batch <= 0 || mode < MVS_CONV_S1 || mode > MVS_CONV_T2) return MVS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 3; ++k)
    if (out_size[k] <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((flags & MVS_CONV_T2_LDS) && mode != MVS_CONV_T2) return MVS_ERR_INVALID_ARGUMENT;
  return mvs::conv3d_region_split_slots(mode, batch, c_in, c_out, out_size, (flags & MVS_CONV_PER_LANE) != 0,
                                        (flags & MVS_CONV_SUM_INPUT) != 0, (flags & MVS_CONV_IN_BN) != 0,
                                        (flags & MVS_CONV_T2_LDS) != 0);
}


int mvs_softmax_depth_fwd(const float* x, int batch, int d_count, int h, int w, float* y, void* stream) {
  if (!x || !y || batch <= 0 || d_count <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)h * (uint64_t)w >= (1ull << 32) || (uint64_t)batch * h * w >= (1ull << 37)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_softmax_depth(x, batch, d_count, (uint32_t)((uint64_t)h * w), y, (hipStream_t)stream);
  return lc.status();
}

int mvs_depth_hypotheses_fwd(const float* d_min, const float* d_int, int batch, int d_num, float d_scale, float* out,
                             void* stream) {
  if (!d_min || !d_int || !out || batch <= 0 || d_num <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((int64_t)batch * d_num >= (1ll << 31)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_depth_hypotheses(d_min, d_int, d_scale, batch, d_num, out, (hipStream_t)stream);
  return lc.status();
}

int mvs_refine_input_fwd(const float* initial_depth, const float* d_min, const float* d_int, int batch, int h,
                         int w, int d_num, float d_scale, const float* ref_img, float* out, void* stream) {
  if (!initial_depth || !d_min || !d_int || !ref_img || !out || batch <= 0 || h <= 0 || w <= 0 || d_num <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)h * (uint64_t)w >= (1ull << 32) || (uint64_t)batch * h * w >= (1ull << 37)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_refine_input(initial_depth, d_min, d_int, d_num, d_scale, ref_img, batch, (uint32_t)((uint64_t)h * w),
                           out, (hipStream_t)stream);
  return lc.status();
}

int mvs_refine_output_fwd(const float* conv, const float* refine_in, const float* d_min, const float* d_int,
                          int batch, int h, int w, int d_num, float d_scale, float* out, void* stream) {
  if (!conv || !refine_in || !d_min || !d_int || !out || batch <= 0 || h <= 0 || w <= 0 || d_num <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)h * (uint64_t)w >= (1ull << 32) || (uint64_t)batch * h * w >= (1ull << 37)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_refine_output(conv, refine_in, d_min, d_int, d_num, d_scale, batch, (uint32_t)((uint64_t)h * w), out,
                            (hipStream_t)stream);
  return lc.status();
}

static bool channel_layout_ok(int layout, int channels, const void* a, const void* b, const void* c) {
  if (layout & ~MVS_LAYOUT_CHANNELS_LAST) return false;
  if (!(layout & MVS_LAYOUT_CHANNELS_LAST)) return true;
  const int c4 = channels / 4;
  if (channels % 4 || c4 > 64 || (c4 & (c4 - 1))) return false;   // quads per voxel: a power of two
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15u) == 0;
}

size_t mvs_channel_stats_slots(int layout, int batch, int channels, long long voxels) {
  if (batch <= 0 || channels <= 0 || voxels <= 0 || (layout & ~MVS_LAYOUT_CHANNELS_LAST)) return 0;
  return mvs::channel_stats_slots((layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, (size_t)voxels);
}

int mvs_channel_stats(const float* x, int layout, int batch, int channels, long long voxels, double* stats,
                      void* stream) {
  if (!x || !stats || batch <= 0 || channels <= 0 || voxels <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if (!channel_layout_ok(layout, channels, x, nullptr, nullptr)) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)batch * channels > 65535u && !(layout & MVS_LAYOUT_CHANNELS_LAST)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_channel_stats(x, (layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, (size_t)voxels, stats,
                            (hipStream_t)stream);
  return lc.status();
}

int mvs_bn_train_params(const double* sums, int channels, double count, const double* border_u,
                        const double* border_count, int prev_channels, int classes, const float* prev_params,
                        const float* weight, const float* bias, float* running_mean, float* running_var,
                        long long* num_batches_tracked, double momentum, double eps, float* params, void* stream) {
  if (!sums || !weight || !bias || !params || channels <= 0 || !(count > 0.0) || !(eps >= 0.0))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!both_or_neither(running_mean, running_var)) return MVS_ERR_INVALID_ARGUMENT;
  if (border_u && (!border_count || !prev_params || prev_channels <= 0 || prev_channels > 256 || classes <= 0 ||
                   (long long)channels * classes > 2048))
    return MVS_ERR_INVALID_ARGUMENT;
  const mvs::LaunchCheck lc;
  mvs::launch_bn_train_params(sums, channels, count, border_u, border_count, prev_channels, classes, prev_params,
                              weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, params,
                              (hipStream_t)stream);
  return lc.status();
}

int mvs_bn_relu(const float* x, int layout, int batch, int channels, long long voxels, const float* scale,
                const float* shift, const float* mean, const float* r, const float* r_scale,
                const float* r_shift, const float* r_mean, float* y, unsigned* y_bound, void* stream) {
  if (!x || !y || !scale || !shift || !mean || batch <= 0 || channels <= 0 || voxels <= 0)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((uintptr_t)y_bound & 3u) return MVS_ERR_INVALID_ARGUMENT;
  if (r && (!r_scale || !r_shift || !r_mean)) return MVS_ERR_INVALID_ARGUMENT;
  if (!channel_layout_ok(layout, channels, x, r, y)) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)batch * channels > 65535u && !(layout & MVS_LAYOUT_CHANNELS_LAST)) return MVS_ERR_TOO_LARGE;
  const mvs::LaunchCheck lc;
  mvs::launch_bn_relu(x, (layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, (size_t)voxels, scale, shift,
                      mean, r, r_scale, r_shift, r_mean, y, reinterpret_cast<uint32_t*>(y_bound),
                      (hipStream_t)stream);
  return lc.status();
}

// ---- training extension: the train-mode BatchNorm + ReLU backward (bn_train_bwd.hip) ----
namespace {
// MVS_OK when the mvs_bn_relu_bwd_* launches can run on this geometry; box: the box's origin and size, or the
// whole volume when both are null
int bn_bwd_geometry(int layout, int batch, int channels, const int* dims, const int* box_origin,
                    const int* box_size, int (&o)[3], int (&s)[3]) {
  if (!dims || batch <= 0 || channels <= 0 || !both_or_neither(box_origin, box_size)) return MVS_ERR_INVALID_ARGUMENT;
  if (!channel_layout_ok(layout, channels, nullptr, nullptr, nullptr)) return MVS_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] <= 0) return MVS_ERR_INVALID_ARGUMENT;
    o[k] = box_origin ? box_origin[k] : 0;
    s[k] = box_size ? box_size[k] : dims[k];
    if (o[k] < 0 || s[k] <= 0 || s[k] > dims[k] || o[k] > dims[k] - s[k]) return MVS_ERR_INVALID_ARGUMENT;
  }
  if ((uint64_t)batch * channels > 65535u && !(layout & MVS_LAYOUT_CHANNELS_LAST)) return MVS_ERR_TOO_LARGE;
  return MVS_OK;
}
}  // namespace

size_t mvs_bn_relu_bwd_slots(int layout, int batch, int channels, const int* dims, const int* box_origin,
                             const int* box_size) {
  int o[3], s[3];
  if (bn_bwd_geometry(layout, batch, channels, dims, box_origin, box_size, o, s) != MVS_OK) return 0;
  return mvs::bn_relu_bwd_slots((layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, dims, s);
}

int mvs_bn_relu_bwd_reduce(const float* z, const float* gy, int layout, int batch, int channels, const int* dims,
                           const int* box_origin, const int* box_size, const float* scale, const float* shift,
                           const float* mean, double* stats, void* stream) {
  if (!z || !gy || !scale || !shift || !mean || !stats) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)z | (uintptr_t)gy) & 15u || (uintptr_t)stats & 7u) return MVS_ERR_INVALID_ARGUMENT;
  int o[3], s[3];
  const int st = bn_bwd_geometry(layout, batch, channels, dims, box_origin, box_size, o, s);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_bn_relu_bwd_reduce(z, gy, (layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, dims, o, s, scale,
                                 shift, mean, stats, (hipStream_t)stream);
  return lc.status();
}

int mvs_bn_relu_bwd_apply(const float* z, const float* gy, int layout, int batch, int channels, const int* dims,
                          const int* box_origin, const int* box_size, const float* scale, const float* shift,
                          const float* mean, const float* g_s1, const float* g_s2, float* gz, void* stream) {
  if (!z || !gy || !scale || !shift || !mean || !g_s1 || !g_s2 || !gz) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)z | (uintptr_t)gy | (uintptr_t)gz) & 15u) return MVS_ERR_INVALID_ARGUMENT;
  int o[3], s[3];
  const int st = bn_bwd_geometry(layout, batch, channels, dims, box_origin, box_size, o, s);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_bn_relu_bwd_apply(z, gy, (layout & MVS_LAYOUT_CHANNELS_LAST) != 0, batch, channels, dims, o, s, scale,
                                shift, mean, g_s1, g_s2, gz, (hipStream_t)stream);
  return lc.status();
}

// ---- training extension: the objective and the depth accuracy (loss.hip; include/train/mvs_loss.h) ----
namespace {
// MVS_OK when the mvs_masked_mae_* launches can run on these dimensions
int masked_mae_geometry(int batch, int h, int w) {
  if (batch <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)h * (uint64_t)w >= (1ull << 31) || batch > 65535) return MVS_ERR_TOO_LARGE;   // counts; grid.y
  return MVS_OK;
}
}  // namespace

int mvs_masked_mae_plan(int batch, int h, int w, int* workgroups, int* passes) {
  const int st = masked_mae_geometry(batch, h, w);
  if (st != MVS_OK) return st;
  const mvs::MaskedMaePlan p = mvs::masked_mae_plan(batch, (size_t)h * (size_t)w);
  if (workgroups) *workgroups = p.workgroups;
  if (passes) *passes = p.passes;
  return MVS_OK;
}

size_t mvs_masked_mae_workspace_bytes(int batch, int h, int w) {
  if (masked_mae_geometry(batch, h, w) != MVS_OK) return 0;
  return (size_t)mvs::masked_mae_plan(batch, (size_t)h * (size_t)w).workgroups * (size_t)batch * 5 * 8;
}

int mvs_masked_mae_fwd(const float* gt, const float* initial, const float* refined, int batch, int h, int w,
                       float thresh, float* loss0, float* loss1, float* acc0, float* acc1, float* n_valid,
                       void* workspace, void* stream) {
  if (!gt || !initial || !refined || !loss0 || !loss1 || !acc0 || !acc1 || !n_valid || !workspace)
    return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)gt | (uintptr_t)initial | (uintptr_t)refined | (uintptr_t)loss0 | (uintptr_t)loss1 |
       (uintptr_t)acc0 | (uintptr_t)acc1 | (uintptr_t)n_valid) & 3u || (uintptr_t)workspace & 7u)
    return MVS_ERR_INVALID_ARGUMENT;
  if (!(thresh >= 0.0f)) return MVS_ERR_INVALID_ARGUMENT;   // (negative or NaN)
  const int st = masked_mae_geometry(batch, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_masked_mae_fwd(gt, initial, refined, batch, (size_t)h * (size_t)w, thresh, loss0, loss1, acc0, acc1,
                             n_valid, static_cast<unsigned long long*>(workspace), (hipStream_t)stream);
  return lc.status();
}

int mvs_masked_mae_bwd(const float* gt, const float* initial, const float* refined, const float* c0, const float* c1,
                       int batch, int h, int w, float* g_initial, float* g_refined, void* stream) {
  if (!gt || !initial || !refined || !c0 || !c1 || !g_initial || !g_refined) return MVS_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)gt | (uintptr_t)initial | (uintptr_t)refined | (uintptr_t)c0 | (uintptr_t)c1 |
       (uintptr_t)g_initial | (uintptr_t)g_refined) & 3u)
    return MVS_ERR_INVALID_ARGUMENT;
  const int st = masked_mae_geometry(batch, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_masked_mae_bwd(gt, initial, refined, c0, c1, batch, (size_t)h * (size_t)w, g_initial, g_refined,
                             (hipStream_t)stream);
  return lc.status();
}

// ---- depth-map filtering and fusion (depth_filter.hip; include/fusion/mvs_depth_filter.h) ----
namespace {
inline bool aligned4(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!p || ((uintptr_t)p & 3u)) return false;
  return true;
}
// MVS_OK when `count` maps of h x w can be indexed by the one-thread-per-pixel launches
int filter_maps_geometry(int count, int h, int w) {
  if (count <= 0 || h <= 0 || w <= 0) return MVS_ERR_INVALID_ARGUMENT;
  const uint64_t hw = (uint64_t)h * (uint64_t)w;
  if (hw >= (1ull << 31) || (uint64_t)count * hw >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  return MVS_OK;
}
int filter_pairs_geometry(int n_views, int n_slots) {
  if (n_views <= 0 || n_slots <= 0 || n_slots > MVS_FILTER_MAX_SLOTS) return MVS_ERR_INVALID_ARGUMENT;
  if ((uint64_t)n_views * (uint64_t)n_slots >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  return MVS_OK;
}
}  // namespace

int mvs_photometric_confidence_fwd(const float* prob, const float* depth, const float* d_batch, int batch, int d_num,
                                   int h, int w, float* conf, void* stream) {
  if (!aligned4({prob, depth, d_batch, conf}) || d_num < 2) return MVS_ERR_INVALID_ARGUMENT;
  const int st = filter_maps_geometry(batch, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_photometric_confidence(prob, depth, d_batch, batch, d_num, (uint32_t)h * (uint32_t)w, conf,
                                     (hipStream_t)stream);
  return lc.status();
}

size_t mvs_view_pair_matrices_bytes(int n_views, int n_slots) {
  if (filter_pairs_geometry(n_views, n_slots) != MVS_OK) return 0;
  return (size_t)n_views * (size_t)n_slots * MVS_FILTER_PAIR_DOUBLES * sizeof(double);
}

int mvs_view_pair_matrices(const float* K, const float* R, const float* T, const int* pairs, int n_views,
                           int n_slots, double* matrices, void* stream) {
  if (!aligned4({K, R, T, pairs}) || !matrices || ((uintptr_t)matrices & 7u)) return MVS_ERR_INVALID_ARGUMENT;
  const int st = filter_pairs_geometry(n_views, n_slots);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_view_pair_matrices(K, R, T, pairs, n_views, n_slots, matrices, (hipStream_t)stream);
  return lc.status();
}

int mvs_geometric_consistency_fwd(const float* depth, const int* pairs, const double* matrices, int n_views,
                                  int n_slots, int h, int w, double px_thresh, double rel_thresh, int* n_consistent,
                                  float* depth_avg, void* stream) {
  if (!aligned4({depth, pairs, n_consistent, depth_avg}) || !matrices || ((uintptr_t)matrices & 7u))
    return MVS_ERR_INVALID_ARGUMENT;
  if (!(px_thresh > 0.0 && std::isfinite(px_thresh) && rel_thresh > 0.0 && std::isfinite(rel_thresh)))
    return MVS_ERR_INVALID_ARGUMENT;
  int st = filter_pairs_geometry(n_views, n_slots);
  if (st == MVS_OK) st = filter_maps_geometry(n_views, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_geometric_consistency(depth, pairs, matrices, n_views, n_slots, h, w, px_thresh, rel_thresh,
                                    n_consistent, depth_avg, (hipStream_t)stream);
  return lc.status();
}

int mvs_backproject_fwd(const float* depth, const float* K, const float* R, const float* T, int n_views, int h,
                        int w, float* xyz, void* stream) {
  if (!aligned4({depth, K, R, T, xyz})) return MVS_ERR_INVALID_ARGUMENT;
  const int st = filter_maps_geometry(n_views, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_backproject(depth, K, R, T, n_views, h, w, xyz, (hipStream_t)stream);
  return lc.status();
}

// ---- the fused point cloud (depth_fuse.hip; include/fusion/mvs_view_fusion.h) ----
size_t mvs_fuse_views_workspace_bytes(int n_views, int h, int w) {
  if (filter_maps_geometry(n_views, h, w) != MVS_OK) return 0;
  return (size_t)n_views * (size_t)h * (size_t)w;
}

int mvs_fuse_views_fwd(const float* depth, const unsigned char* mask, const float* colors, const float* K,
                       const float* R, const float* T, const int* pairs, const double* matrices, int n_views,
                       int n_slots, int h, int w, double px_thresh, double rel_thresh, unsigned char* used,
                       unsigned char* emitted, int* n_merged, float* xyz, float* rgb, void* stream) {
  if (!aligned4({depth, K, R, T, pairs, n_merged, xyz}) || !matrices || ((uintptr_t)matrices & 7u) || !mask ||
      !used || !emitted)
    return MVS_ERR_INVALID_ARGUMENT;
  if ((colors == nullptr) != (rgb == nullptr) || (colors && !aligned4({colors, rgb}))) return MVS_ERR_INVALID_ARGUMENT;
  if (!(px_thresh > 0.0 && std::isfinite(px_thresh) && rel_thresh > 0.0 && std::isfinite(rel_thresh)))
    return MVS_ERR_INVALID_ARGUMENT;
  int st = filter_pairs_geometry(n_views, n_slots);
  if (st == MVS_OK) st = filter_maps_geometry(n_views, h, w);
  if (st != MVS_OK) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_fuse_views(depth, mask, colors, K, R, T, pairs, matrices, n_views, n_slots, h, w, px_thresh,
                         rel_thresh, used, emitted, n_merged, xyz, rgb, (hipStream_t)stream);
  return lc.status();
}

}  // extern "C"

// ---- nearest-neighbour distances between two clouds (cloud_nn.hip; include/fusion/mvs_cloud_eval.h) ----
namespace {
int cloud_count(long long n) {
  if (n < 0) return MVS_ERR_INVALID_ARGUMENT;
  return n >= (1ll << 31) ? MVS_ERR_TOO_LARGE : MVS_OK;
}
// MVS_OK for a grid the kernels can index: dimensions >= 1, at most MVS_CLOUD_MAX_CELLS cells
int cloud_grid_geometry(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1) return MVS_ERR_INVALID_ARGUMENT;
  const uint64_t cells = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;   // (read only once nx ny < 2^31: no wrap)
  if ((uint64_t)nx * (uint64_t)ny >= (1ull << 31) || cells >= (1ull << 31)) return MVS_ERR_TOO_LARGE;
  return cells > (uint64_t)MVS_CLOUD_MAX_CELLS ? MVS_ERR_INVALID_ARGUMENT : MVS_OK;
}
int cloud_grid_ok(double ox, double oy, double oz, double cell, int nx, int ny, int nz) {
  if (!(std::isfinite(ox) && std::isfinite(oy) && std::isfinite(oz) && cell > 0.0 && std::isfinite(cell)))
    return MVS_ERR_INVALID_ARGUMENT;
  return cloud_grid_geometry(nx, ny, nz);
}
}  // namespace

extern "C" {

size_t mvs_cloud_cell_table_bytes(int nx, int ny, int nz) {
  if (cloud_grid_geometry(nx, ny, nz) != MVS_OK) return 0;
  return ((size_t)nx * (size_t)ny * (size_t)nz + 1) * sizeof(int);
}

int mvs_cloud_cell_keys(const float* points, long long n, double origin_x, double origin_y, double origin_z,
                        double cell, int nx, int ny, int nz, int* keys, void* stream) {
  if (!aligned4({points, keys})) return MVS_ERR_INVALID_ARGUMENT;
  int st = cloud_count(n);
  if (st == MVS_OK) st = cloud_grid_ok(origin_x, origin_y, origin_z, cell, nx, ny, nz);
  if (st != MVS_OK || n == 0) return st;
  const mvs::LaunchCheck lc;
  mvs::launch_cloud_cell_keys(points, (int)n, origin_x, origin_y, origin_z, cell, nx, ny, nz, keys,
                              (hipStream_t)stream);
  return lc.status();
}

int mvs_cloud_cell_ranges(const int* sorted_keys, long long n, long long ncells, int* cell_start, void* stream) {
  if (!aligned4({sorted_keys, cell_start})) return MVS_ERR_INVALID_ARGUMENT;
  int st = cloud_count(n);
  if (st == MVS_OK) st = cloud_count(ncells);
  if (st != MVS_OK) return st;
  if (ncells < 1 || ncells > MVS_CLOUD_MAX_CELLS) return MVS_ERR_INVALID_ARGUMENT;
  const mvs::LaunchCheck lc;
  mvs::launch_cloud_cell_ranges(sorted_keys, (int)n, (int)ncells, cell_start, (hipStream_t)stream);
  return lc.status();
}

int mvs_cloud_nearest(const float* query, const int* query_order, long long m, const float* targets,
                      const int* target_index, long long g, const int* cell_start, double origin_x, double origin_y,
                      double origin_z, double cell, int nx, int ny, int nz, double max_dist, float* dist, int* index,
                      void* stream) {
  if (!aligned4({query, query_order, targets, target_index, cell_start, dist, index})) return MVS_ERR_INVALID_ARGUMENT;
  int st = cloud_count(m);
  if (st == MVS_OK) st = cloud_count(g);
  if (st == MVS_OK) st = cloud_grid_ok(origin_x, origin_y, origin_z, cell, nx, ny, nz);
  if (st != MVS_OK) return st;
  if (!(max_dist > 0.0 && std::isfinite(max_dist))) return MVS_ERR_INVALID_ARGUMENT;
  const double rings = std::ceil(max_dist / cell);
  if (!(rings <= (double)MVS_CLOUD_MAX_RINGS)) return MVS_ERR_INVALID_ARGUMENT;
  if (m == 0) return MVS_OK;
  const mvs::LaunchCheck lc;
  mvs::launch_cloud_nearest(query, query_order, (int)m, targets, target_index, (int)g, cell_start, origin_x, origin_y,
                            origin_z, cell, nx, ny, nz, (int)rings, max_dist, dist, index, (hipStream_t)stream);
  return lc.status();
}

}  // extern "C"
