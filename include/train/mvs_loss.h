/* mvs_loss.h -- training extension of libmvs_cost_volume.so: the training objective of the reference's loss.py
 * (loss_fcn, loss.py:4-41) and the depth accuracy its config.py:4 defines (ACC_THRESH), forward and backward
 * (mvs_amd/loss.py; kernels: csrc/loss.hip).
 *
 * Additive, like mvs_region_train.h, and under the same MVS_TRAIN_ABI_VERSION.  Status codes, pointer and stream
 * conventions are those of mvs_cost_volume.h: every pointer is a DEVICE pointer unless stated, `stream` is a
 * hipStream_t (NULL: the default stream), nothing allocates or synchronises.
 */
#ifndef MVS_LOSS_H
#define MVS_LOSS_H

#include <stddef.h>

#include "../mvs_cost_volume.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gt, initial, refined: [batch][1][h][w] contiguous fp32 depth maps (4-byte aligned; 16-byte accesses are used for
 * every sample whose three base addresses are 16-byte aligned, scalar ones otherwise -- the results are the same
 * bits either way).  A pixel is valid where gt != 0 (a NaN gt is valid, as torch.ne).  Per sample b, over its valid
 * pixels:
 *   n_valid[b] = their number
 *   loss0[b]   = (float)(sum |gt - initial|) / (float)n_valid     the sum and its terms in float64, one fp32 division;
 *   loss1[b]     alike for refined                                0 / 0 = NaN for a sample without a valid pixel
 *   acc0[b]    = #{|gt - initial| <= thresh * |gt|} / n_valid     fp32 difference, one fp32 product; a NaN difference
 *   acc1[b]      alike for refined                                is not accurate
 * each a [batch] fp32 vector.  One pass over the three maps: every workgroup writes its own partial sums (float64)
 * and counts (64-bit) to its slot of the workspace, a second small kernel adds the slots in slot order: no atomics,
 * nothing zeroed, bit-reproducible whatever the workspace held.
 *   plan:      *workgroups = workgroups per sample (the grid is workgroups x batch; at most about 1024 in all),
 *              *passes = the grid-stride passes each makes over the sample's ceil(h w / 4) four-element items;
 *              either pointer may be null.  Returns the status the forward would (dimensions only).
 *   workspace: mvs_masked_mae_workspace_bytes(batch, h, w) = workgroups * batch * 5 * 8 bytes (0 for arguments the
 *              launch would refuse), 8-byte aligned.
 * MVS_ERR_INVALID_ARGUMENT: a null or misaligned pointer, batch <= 0, h <= 0, w <= 0, thresh negative or NaN.
 * MVS_ERR_TOO_LARGE: h * w >= 2^31 or batch > 65535.  Arguments are checked before any launch. */
int mvs_masked_mae_plan(int batch, int h, int w, int* workgroups, int* passes);
size_t mvs_masked_mae_workspace_bytes(int batch, int h, int w);
int mvs_masked_mae_fwd(const float* gt, const float* initial, const float* refined, int batch, int h, int w,
                       float thresh, float* loss0, float* loss1, float* acc0, float* acc1, float* n_valid,
                       void* workspace, void* stream);

/* Both gradients of the forward's loss0 / loss1 in one pass over the three maps:
 *   g_initial[b][e] = -((c0[b] * m) * sgn(gt - initial)),  m = 1 where gt != 0 and 0 elsewhere;  g_refined with c1
 * c0, c1: [batch] fp32, the upstream gradients of loss0 / loss1 divided by n_valid (the caller's [batch]-sized ops).
 * These are the products torch's autograd of the reference expression forms, in its order: 0 where gt = 0 or the two
 * depths tie, 0 * inf = NaN at every pixel of a sample without a valid pixel; sgn(x) = (0 < x) - (x < 0) as
 * torch.sign, 0 for a NaN.  g_initial, g_refined: [batch][1][h][w] fp32, every element written once.  Pointers and
 * dimensions as above. */
int mvs_masked_mae_bwd(const float* gt, const float* initial, const float* refined, const float* c0, const float* c1,
                       int batch, int h, int w, float* g_initial, float* g_refined, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MVS_LOSS_H */
