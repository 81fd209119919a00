/* mvs_region_train.h -- training extension of libmvs_cost_volume.so: entry points that only the
 * autograd backward of the regulariser's region convolutions uses (mvs_amd/region_train.py).
 *
 * This surface is additive and versioned on its own (MVS_TRAIN_ABI_VERSION): the drop-in contract of
 * include/mvs_cost_volume.h (MVS_ABI_VERSION) does not change when it grows.  Status codes, pointer and
 * stream conventions are those of mvs_cost_volume.h: every pointer is a DEVICE pointer unless stated,
 * `stream` is a hipStream_t (NULL: the default stream), nothing allocates or synchronises.
 */
#ifndef MVS_REGION_TRAIN_H
#define MVS_REGION_TRAIN_H

#include <stddef.h>

#include "../mvs_cost_volume.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_TRAIN_ABI_VERSION 1   /* added entry points do not bump it: only a changed one would */

/* Training-extension ABI version of the loaded library (MVS_TRAIN_ABI_VERSION at build time). */
int mvs_train_abi_version(void);

/* Weight gradient of a stride-1 region convolution nn.Conv3d(C, C, 3, padding=0, bias=False) applied to
 * the zero-padded crop (model.py:108-113 conv_1_1 / conv_2_1 / conv_3_1 through _conv_s1_region):
 *   dw[co][ci][tz][ty][tx] = sum over b and every output voxel o of gy[b][o][co] * x[b][o + t][ci]
 * fp32 products and sums on the f32-input matrix cores, partial sums per workgroup reduced in a fixed
 * order (bit-reproducible; no atomics; the workspace need not be zeroed).
 *   x  [batch][Lz][Ly][Lx][channels]            channels-last padded crop, in_size = {Lz, Ly, Lx} (HOST)
 *   gy [batch][Lz-2][Ly-2][Lx-2][channels]      channels-last output gradient
 *   dw [channels][channels][3][3][3]            nn.Conv3d's weight layout
 * x, gy, dw and workspace contiguous fp32 with 16-byte-aligned bases; channels in {16, 32, 64}; every
 * in_size[k] >= 3; batch * Lz * Ly * Lx < 2^31 (else MVS_ERR_TOO_LARGE).
 * workspace: mvs_conv3d_region_wgrad_workspace_bytes(batch, channels, in_size) bytes (0 for arguments
 * the launch would refuse). */
size_t mvs_conv3d_region_wgrad_workspace_bytes(int batch, int channels, const int* in_size);
int mvs_conv3d_region_wgrad(const float* x, const float* gy, int batch, int channels, const int* in_size,
                            float* dw, float* workspace, void* stream);

/* Backward of the stacked stride-2 region convolution nn.Conv3d(32, 112, 3, stride=2, bias=False) of the whole
 * cost volume on an output box (model.py:101-107 conv_1_0 / conv_2_0 / conv_3_0 stacked 16 + 32 + 64 through
 * _conv_s2_region): output voxel o reads inputs 2 * o - pad_lo + t per dim, t = 0..2, inputs off the volume
 * are 0.  The channel counts are FIXED: 32 in, 112 out.
 *   x   [batch][32][D][H][W]            the volume, NCDHW, read in place; dims = {D, H, W} (HOST int[3])
 *   gy  [batch][Oz][Oy][Ox][112]        channels-last output gradient; out_size = {Oz, Oy, Ox} (HOST int[3])
 *   dw  [112][32][3][3][3]              nn.Conv3d's weight layout
 *   w27 [27][32][112]                   the weight as [tap][ci][co]
 *   gx  [batch][32][D][H][W]            NCDHW, every element written
 * pad_lo (HOST int[3]): every pad_lo[k] >= 0, dims[k] >= 1, out_size[k] >= 1; every device pointer
 * contiguous fp32 with a 16-byte-aligned base.  batch * D * H * W and batch * Oz * Oy * Ox below 2^31 and
 * one sample of gy below 4 GB (else MVS_ERR_TOO_LARGE).
 *   wgrad: dw[co][ci][t] = sum over b and o of gy[b][o][co] * x[b][2 o - pad_lo + t][ci]: fp32 on the
 *          f32-input matrix cores, partial sums per workgroup reduced in a fixed order (bit-reproducible; no
 *          atomics; the workspace need not be zeroed).  workspace:
 *          mvs_conv3d_s2_region_wgrad_workspace_bytes(batch, dims, out_size) bytes (0 for arguments the
 *          launch would refuse).
 *   dgrad: gx[b][ci][i] = sum over t and co of gy[b][(i + pad_lo - t) / 2][co] * w[co][ci][t] over the t with
 *          i + pad_lo - t even and the quotient inside the box: four partial sums per output (gy channels
 *          0-15 | 16-47 | 48-79 | 80-111), added once as (p0 + p1) + (p2 + p3). */
size_t mvs_conv3d_s2_region_wgrad_workspace_bytes(int batch, const int* dims, const int* out_size);
int mvs_conv3d_s2_region_wgrad(const float* x, const float* gy, int batch, const int* dims, const int* pad_lo,
                               const int* out_size, float* dw, float* workspace, void* stream);
int mvs_conv3d_s2_region_dgrad(const float* gy, const float* w27, int batch, const int* dims, const int* pad_lo,
                               const int* out_size, float* gx, void* stream);

/* Backward of a transposed region convolution nn.ConvTranspose3d(c_in, c_out, 3, stride=2, bias=False) on an
 * output box (model.py:117-120 deconv_3_0 / deconv_2_0 through _tconv_region): the box holds outputs
 * [crop, crop + out_size) of the unpadded transposed convolution, input voxel i reaches box output
 * 2 * i - crop + t per dim, t = 0..2; taps that land outside the box are dropped.  (c_in, c_out) is (64, 32)
 * or (32, 16): anything else is MVS_ERR_INVALID_ARGUMENT.
 *   x   [batch][Iz][Iy][Ix][c_in]       channels-last input; in_size = {Iz, Iy, Ix} (HOST int[3])
 *   gy  [batch][Oz][Oy][Ox][c_out]      channels-last output gradient, read in place; out_size (HOST int[3])
 *   dw  [c_in][c_out][3][3][3]          nn.ConvTranspose3d's weight layout
 *   w27 [27][c_in][c_out]               the weight as [tap][ci][co]
 *   gx  [batch][Iz][Iy][Ix][c_in]       channels-last, every element written
 * crop (HOST int[3]): every crop[k] >= 0, in_size[k] >= 1, out_size[k] >= 1; every device pointer contiguous
 * fp32 with a 16-byte-aligned base.  batch * Iz * Iy * Ix and batch * Oz * Oy * Ox below 2^31 and one sample of
 * gy below 4 GB (else MVS_ERR_TOO_LARGE).
 *   wgrad: dw[ci][co][t] = sum over b and i of x[b][i][ci] * gy[b][2 i - crop + t][co]: fp32 on the f32-input
 *          matrix cores, partial sums per workgroup reduced in a fixed order (bit-reproducible; no atomics; the
 *          workspace need not be zeroed).  workspace:
 *          mvs_conv3d_t2_region_wgrad_workspace_bytes(batch, c_in, c_out, in_size, out_size) bytes (0 for
 *          arguments the launch would refuse).
 *   dgrad: gx[b][i][ci] = sum over t and co of gy[b][2 i - crop + t][co] * w[ci][co][t]: three partial sums per
 *          output, one per tap plane tz, added once as (p0 + p1) + p2. */
size_t mvs_conv3d_t2_region_wgrad_workspace_bytes(int batch, int c_in, int c_out, const int* in_size,
                                                  const int* out_size);
int mvs_conv3d_t2_region_wgrad(const float* x, const float* gy, int batch, int c_in, int c_out, const int* in_size,
                               const int* crop, const int* out_size, float* dw, float* workspace, void* stream);
int mvs_conv3d_t2_region_dgrad(const float* gy, const float* w27, int batch, int c_in, int c_out, const int* in_size,
                               const int* crop, const int* out_size, float* gx, void* stream);

/* Backward of the last transposed region convolution nn.ConvTranspose3d(16, 8, 3, stride=2, bias=False) on an
 * output box (model.py:121 deconv_1_0 through _tconv_region; its forward is mvs_deconv3d_k3s2_fwd without BN and
 * residual, with pad - 2 * origin = crop per dim): the box holds outputs [crop, crop + out_size) of the unpadded
 * transposed convolution, input voxel i reaches box output 2 * i - crop + t per dim, t = 0..2; taps that land
 * outside the box are dropped.  (c_in, c_out) must be (16, 8): anything else is MVS_ERR_INVALID_ARGUMENT.
 *   x   [batch][16][Iz][Iy][Ix]         the input, NCDHW, or with flags = MVS_LAYOUT_CHANNELS_LAST
 *                                       [batch][Iz][Iy][Ix][16]; in_size = {Iz, Iy, Ix} (HOST int[3])
 *   gy  [batch][8][Oz][Oy][Ox]          NCDHW output gradient, read in place; out_size (HOST int[3])
 *   dw  [16][8][3][3][3]                nn.ConvTranspose3d's weight layout
 *   w27 [27][16][8]                     the weight as [tap][ci][co]
 *   gx  x's layout (flags), every element written
 * flags: 0 or MVS_LAYOUT_CHANNELS_LAST.  crop (HOST int[3]): every crop[k] >= 0, in_size[k] >= 1,
 * out_size[k] >= 1; every device pointer contiguous fp32 with a 16-byte-aligned base.  Index width: batch * Iz *
 * Iy * Ix and batch * Oz * Oy * Ox below 2^31, every in_size[k] and crop[k] below 2^29, and one sample of gy
 * (8 * Oz * Oy * Ox floats) below 4 GB (else MVS_ERR_TOO_LARGE); gy as a whole may pass 4 GB.
 *   wgrad: dw[ci][co][t] = sum over b and i of x[b][ci][i] * gy[b][co][2 i - crop + t]: fp32 on the f32-input
 *          matrix cores, partial sums per workgroup reduced in a fixed order (bit-reproducible; no atomics; the
 *          workspace need not be zeroed).  workspace:
 *          mvs_deconv3d_k3s2_wgrad_workspace_bytes(batch, c_in, c_out, in_size, out_size) bytes (0 for arguments
 *          the launch would refuse).
 *   dgrad: gx[b][ci][i] = sum over t and co of gy[b][co][2 i - crop + t] * w[ci][co][t]: one output owner per
 *          input voxel, three partial sums per output, one per tap plane tz, added once as (p0 + p1) + p2. */
size_t mvs_deconv3d_k3s2_wgrad_workspace_bytes(int batch, int c_in, int c_out, const int* in_size,
                                               const int* out_size);
int mvs_deconv3d_k3s2_wgrad(const float* x, int flags, const float* gy, int batch, int c_in, int c_out,
                            const int* in_size, const int* crop, const int* out_size, float* dw, float* workspace,
                            void* stream);
int mvs_deconv3d_k3s2_dgrad(const float* gy, const float* w27, int flags, int batch, int c_in, int c_out,
                            const int* in_size, const int* crop, const int* out_size, float* gx, void* stream);

/* Backward of a train-mode BatchNorm + ReLU site of the regulariser (mvs_amd/bn_train.py):
 *   out = relu((z[box] - mean) * scale + shift), the batch statistics formed over ALL of z
 * (forward: mvs_channel_stats, mvs_bn_relu on a copy of the box).  Two passes, each reading z and gy once:
 *   reduce: ga = gy where (z - mean) * scale + shift > 0 -- mvs_bn_relu's expression and rounding, so the mask is
 *           the forward's -- and 0 elsewhere; stats[slot][0][c] = sum ga, stats[slot][1][c] = sum ga * z over the
 *           box, float64, one slot per workgroup written once and summed by the caller in slot order
 *           (bit-reproducible; no atomics; stats need not be zeroed).  Slots:
 *           mvs_bn_relu_bwd_slots(...) (0 for arguments the launch would refuse).
 *   apply:  gz = ga * scale + g_s1 + 2 * z * g_s2 over all of z (ga = 0 outside the box), fp32, every element
 *           written once; its grid is the reduce's for the whole volume (mvs_bn_relu_bwd_slots with a null box).
 *   z, gz [batch][channels][D][H][W]        NCDHW, or with layout = MVS_LAYOUT_CHANNELS_LAST
 *                                           [batch][D][H][W][channels]; dims = {D, H, W} (HOST int[3])
 *   gy                                      z's layout on the box: [batch][channels][sz][sy][sx] or
 *                                           [batch][sz][sy][sx][channels], contiguous
 *   scale, shift, mean, g_s1, g_s2 [channels]   fp32 (mvs_bn_train_params' rows; the sums' gradients)
 * box_origin, box_size (HOST int[3]): both null (the whole volume) or both given with 0 <= origin and
 * origin + size <= dims, size >= 1 per dim.  Channels-last wants channels = 4 * a power of two <= 256; NCDHW
 * wants batch * channels <= 65535 (else MVS_ERR_TOO_LARGE).  z, gy and gz contiguous fp32 with 16-byte-aligned
 * bases; they may pass 4 GB (64-bit offsets). */
size_t mvs_bn_relu_bwd_slots(int layout, int batch, int channels, const int* dims, const int* box_origin,
                             const int* box_size);
int mvs_bn_relu_bwd_reduce(const float* z, const float* gy, int layout, int batch, int channels, const int* dims,
                           const int* box_origin, const int* box_size, const float* scale, const float* shift,
                           const float* mean, double* stats, void* stream);
int mvs_bn_relu_bwd_apply(const float* z, const float* gy, int layout, int batch, int channels, const int* dims,
                          const int* box_origin, const int* box_size, const float* scale, const float* shift,
                          const float* mean, const float* g_s1, const float* g_s2, float* gz, void* stream);

/* Backward of the 2-D feature encoder's and refinement net's bias-free convolutions nn.Conv2d(c_in, c_out, k,
 * stride, padding = k / 2, bias=False) (model.py:22-65, 134-145; forward: mvs_conv2d_fwd) under autograd
 * (mvs_amd/conv2d_train.py).  (c_in, c_out, k, stride) is one of (3,8,3,1) (8,8,3,1) (8,16,5,2) (16,16,3,1)
 * (16,32,5,2) (32,32,3,1) (4,32,3,1) (32,1,3,1): anything else is MVS_ERR_INVALID_ARGUMENT.
 *   x, gx  [n][c_in][h][w]              NCHW, read / written in place
 *   gy     [n][c_out][ho][wo]           NCHW, ho = (h + 2 (k / 2) - k) / stride + 1, wo alike
 *   weight, dw [c_out][c_in][k][k]      nn.Conv2d's weight layout
 * Every device pointer contiguous fp32 with a 16-byte-aligned base; n, h, w >= 1.  Index width: the element
 * counts of x and of gy below 2^31 (else MVS_ERR_TOO_LARGE; offsets themselves are 64-bit), and for the input
 * gradient n <= 65535 (else MVS_ERR_TOO_LARGE).  Arguments are checked before any launch: a refused call touches
 * no memory.
 *   dgrad: gx[n][ci][iy][ix] = sum over co, ky, kx of weight[co][ci][ky][kx] * gy[n][co][oy][ox] with
 *          oy * stride + ky - k / 2 = iy (x alike): one owner per input pixel, fp32 fmaf chains in the order
 *          co, ky, kx; no atomics, every element of gx written once.
 *   wgrad: dw[co][ci][ky][kx] = sum over n, oy, ox of gy[n][co][oy][ox] * x[n][ci][oy * stride + ky - k / 2][..]:
 *          fp32 on the f32-input matrix cores; persistent workgroups walk the 32 x 8 output tiles (tile t goes to
 *          workgroup t mod slots) and store one partial slot each, written exactly once per launch; the slots are
 *          summed in slot order (bit-reproducible; no atomics; the workspace need not be zeroed).
 *   plan:  *tiles = n * ceil(ho / 8) * ceil(wo / 32), *slots = min(*tiles, 512); either pointer may be null.
 *          Returns the status the weight gradient would (dimensions only).
 *   workspace: mvs_conv2d_wgrad_workspace_bytes(...) = slots * c_in * 16 ceil(k k / 16) * 16 ceil(c_out / 16)
 *          floats (0 for arguments the launch would refuse). */
int mvs_conv2d_wgrad_plan(int n, int c_in, int c_out, int h, int w, int k, int stride, int* tiles, int* slots);
size_t mvs_conv2d_wgrad_workspace_bytes(int n, int c_in, int c_out, int h, int w, int k, int stride);
int mvs_conv2d_wgrad(const float* x, const float* gy, int n, int c_in, int c_out, int h, int w, int k, int stride,
                     float* dw, float* workspace, void* stream);
int mvs_conv2d_dgrad(const float* gy, const float* weight, int n, int c_in, int c_out, int h, int w, int k,
                     int stride, float* gx, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_REGION_TRAIN_H */
