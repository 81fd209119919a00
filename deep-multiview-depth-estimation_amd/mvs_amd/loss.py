"""Drop-in for the reference's scripts/loss.py, and the depth accuracy its config.py:4 defines and never computes.

  loss_fcn(gt, initial, refined) -> (loss, initial_acc, refined_acc)        loss.py:4-41
      mask = gt != 0; per sample the mean absolute error of the initial and of the refined depth map over the valid
      pixels; loss = the sum of both over the batch, the two "accuracies" = the per-sample errors averaged over the
      batch (what the reference's drivers print as "Acc 1 / Acc 2").  Three 0-dim tensors.
  depth_accuracy(gt, initial, refined, thresh=ACC_THRESH) -> (initial_frac, refined_frac)
      the share of valid pixels whose depth is within thresh * |gt| of gt ("correct depth is within ACC_THRESH
      percent of true depth"), per sample, averaged over the batch.  Not differentiable.

fp32 device tensors of shape [B, 1, h, w] run on the HIP kernels of csrc/loss.hip (include/train/mvs_loss.h), under
no_grad and under autograd alike: one pass over the three maps forward (float64 sums in write-once slots, added in
slot order: bit-reproducible), one pass backward for both gradients, and a few [B]-sized torch ops around them.  The
torch expression of the reference is a dozen launches forward and about twenty backward over the same maps.  Calling
these functions is the opt-in: no environment switch selects them and nothing in model.py routes to them.

Anything else (CPU tensors, other dtypes, other shapes) takes the reference's torch expression: a loss has no reason
to refuse a CPU tensor.  gt gets no gradient on the HIP path.

The two ops live in the namespace ``mvs_train`` (the ``mvs`` namespace is the drop-in surface and stays as it is):
  mvs_train::masked_mae(gt, initial, refined, thresh) -> (loss0, loss1, acc0, acc1, n_valid), five fp32 [B]
  mvs_train::masked_mae_bwd(gt, initial, refined, c0, c1) -> (g_initial, g_refined)
The first carries the autograd formula; it saves the three maps and n_valid, nothing else of full size."""
import ctypes
import math
from typing import Tuple

import torch

from . import _lib
from .config import ACC_THRESH
from .ops import _require_gpu

_F32 = torch.float32


def plan(batch, h, w):
    """(workgroups per sample, grid-stride passes of each) of the kernels for these dimensions
    (mvs_masked_mae_plan); ValueError when refused."""
    wg, passes = ctypes.c_int(0), ctypes.c_int(0)
    st = _lib.load().mvs_masked_mae_plan(batch, h, w, ctypes.byref(wg), ctypes.byref(passes))
    if st != _lib.MVS_OK:
        raise ValueError("mvs_masked_mae_plan: %s (%d)" % (_lib.STATUS.get(st, "?"), st))
    return wg.value, passes.value


def _maps(gt, initial, refined, what):
    """The three maps as contiguous fp32 [B, 1, h, w] on gt's device (copies only where they are not already; a
    storage offset that breaks 16-byte alignment is the kernels' scalar path) and (B, h, w)."""
    for t, name in ((gt, "gt"), (initial, "initial"), (refined, "refined")):
        _require_gpu(t, name)
    if gt.dim() != 4 or gt.shape[1] != 1 or initial.shape != gt.shape or refined.shape != gt.shape:
        raise ValueError("%s: three [B, 1, h, w] maps expected, got %s, %s and %s"
                         % (what, tuple(gt.shape), tuple(initial.shape), tuple(refined.shape)))
    if not (gt.dtype == initial.dtype == refined.dtype == _F32) or not (gt.device == initial.device == refined.device):
        raise ValueError("%s: fp32 maps on one device expected" % what)
    return gt.contiguous(), initial.contiguous(), refined.contiguous(), gt.shape[0], gt.shape[2], gt.shape[3]


def _forward(gt, initial, refined, thresh, workspace):
    """masked_mae's body; ``workspace``: None, or device memory of at least the query's size, 8-byte aligned, to use
    as the slots (the tests fill it first)."""
    lib = _lib.load()
    gt, initial, refined, B, h, w = _maps(gt, initial, refined, "masked_mae")
    if not thresh >= 0.0:
        raise ValueError("masked_mae: thresh >= 0 expected, got %r" % (thresh,))
    nbytes = lib.mvs_masked_mae_workspace_bytes(B, h, w)
    if nbytes == 0:
        raise ValueError("masked_mae: maps %s: B in 1..65535 and 0 < h * w < 2^31 expected" % (tuple(gt.shape),))
    if workspace is None:
        workspace = torch.empty(nbytes // 8, device=gt.device, dtype=torch.float64)
    elif workspace.numel() * workspace.element_size() < nbytes or workspace.data_ptr() % 8 \
            or not workspace.is_contiguous() or workspace.device != gt.device:
        raise ValueError("masked_mae: a contiguous 8-byte-aligned workspace of %d bytes expected" % nbytes)
    out = tuple(torch.empty(B, device=gt.device, dtype=_F32) for _ in range(5))
    st = lib.mvs_masked_mae_fwd(_lib.ptr(gt), _lib.ptr(initial), _lib.ptr(refined), B, h, w, thresh,
                                *[_lib.ptr(o) for o in out], _lib.ptr(workspace), _lib.stream_handle(gt.device))
    _lib.check(st, "mvs_masked_mae_fwd")
    return out


@torch.library.custom_op("mvs_train::masked_mae", mutates_args=())
def masked_mae(gt: torch.Tensor, initial: torch.Tensor, refined: torch.Tensor,
               thresh: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(loss0, loss1, acc0, acc1, n_valid), fp32 [B] each, of three fp32 [B, 1, h, w] device maps: per sample the mean
    of |gt - initial| / |gt - refined| over the valid (gt != 0) pixels, the share of them within thresh * |gt|, and
    their number (mvs_masked_mae_fwd).  Differentiable in initial and refined through loss0 / loss1."""
    return _forward(gt, initial, refined, thresh, None)


@masked_mae.register_fake
def _(gt, initial, refined, thresh):
    return tuple(gt.new_empty((gt.shape[0],)) for _ in range(5))


@torch.library.custom_op("mvs_train::masked_mae_bwd", mutates_args=())
def masked_mae_bwd(gt: torch.Tensor, initial: torch.Tensor, refined: torch.Tensor, c0: torch.Tensor,
                   c1: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(g_initial, g_refined) [B, 1, h, w]: -(c[b] * (gt != 0)) * sign(gt - depth) with c0 / c1 [B] fp32, the
    upstream gradients of loss0 / loss1 over n_valid (mvs_masked_mae_bwd).  Every element written."""
    lib = _lib.load()
    gt, initial, refined, B, h, w = _maps(gt, initial, refined, "masked_mae_bwd")
    c0, c1 = (c.to(device=gt.device, dtype=_F32).contiguous() for c in (c0, c1))
    if c0.shape != (B,) or c1.shape != (B,):
        raise ValueError("masked_mae_bwd: c0 and c1 [%d] expected, got %s and %s"
                         % (B, tuple(c0.shape), tuple(c1.shape)))
    g0, g1 = torch.empty_like(initial), torch.empty_like(refined)
    st = lib.mvs_masked_mae_bwd(_lib.ptr(gt), _lib.ptr(initial), _lib.ptr(refined), _lib.ptr(c0), _lib.ptr(c1), B, h, w,
                                _lib.ptr(g0), _lib.ptr(g1), _lib.stream_handle(gt.device))
    _lib.check(st, "mvs_masked_mae_bwd")
    return g0, g1


@masked_mae_bwd.register_fake
def _(gt, initial, refined, c0, c1):
    return torch.empty_like(initial, memory_format=torch.contiguous_format), \
        torch.empty_like(refined, memory_format=torch.contiguous_format)


def _setup_context(ctx, inputs, output):
    gt, initial, refined, _ = inputs
    ctx.save_for_backward(gt, initial, refined, output[4])
    ctx.set_materialize_grads(False)   # (no zero tensors for the outputs nothing was computed from)


def _backward(ctx, g_loss0, g_loss1, g_acc0, g_acc1, g_n):
    """The reference expression's autograd, its [B]-sized part in torch: loss_b = S_b / n_valid_b, so each map's
    gradient is (upstream / n_valid) under the mask and the sign -- one fp32 division per sample, as torch's div
    backward.  acc0, acc1 and n_valid are piecewise constant: their upstream gradients are not used."""
    gt, initial, refined, n_valid = ctx.saved_tensors
    if g_loss0 is None and g_loss1 is None:
        return None, None, None, None
    c0 = (torch.zeros_like(n_valid) if g_loss0 is None else g_loss0) / n_valid
    c1 = (torch.zeros_like(n_valid) if g_loss1 is None else g_loss1) / n_valid
    g0, g1 = masked_mae_bwd(gt, initial, refined, c0, c1)
    return None, (g0 if ctx.needs_input_grad[1] else None), (g1 if ctx.needs_input_grad[2] else None), None


masked_mae.register_autograd(_backward, setup_context=_setup_context)


def _on_hip(gt, initial, refined):
    """The three maps go to the kernels: fp32 [B, 1, h, w] on one HIP device, B and h * w inside the kernels' range."""
    return (all(t.is_cuda and t.dtype == _F32 for t in (gt, initial, refined))
            and gt.dim() == 4 and gt.shape[1] == 1 and initial.shape == gt.shape and refined.shape == gt.shape
            and gt.device == initial.device == refined.device
            and 0 < gt.shape[0] <= 65535 and 0 < gt.shape[2] * gt.shape[3] < 2 ** 31)


def loss_fcn(gt, initial, refined):
    """loss.py:4-41.  (loss, initial_acc, refined_acc), three 0-dim tensors: loss = the sum over the batch of both
    per-sample masked mean absolute errors, the other two = each map's per-sample error averaged over the batch."""
    if _on_hip(gt, initial, refined):
        loss_0, loss_1 = masked_mae(gt.detach(), initial, refined, float(ACC_THRESH))[:2]
    else:
        mask = torch.ne(gt, torch.tensor(0.0, dtype=gt.dtype, device=gt.device)).to(gt.dtype)
        p_valid = mask.sum((1, 2, 3))
        initial_diff = torch.abs(torch.subtract(gt, initial))
        refined_diff = torch.abs(torch.subtract(gt, refined))
        loss_0 = torch.multiply(mask, initial_diff).sum((1, 2, 3)).div(p_valid)
        loss_1 = torch.multiply(mask, refined_diff).sum((1, 2, 3)).div(p_valid)
    return (loss_0 + loss_1).sum(), loss_0.mean(), loss_1.mean()


def depth_accuracy(gt, initial, refined, thresh=ACC_THRESH):
    """(initial_frac, refined_frac), two 0-dim tensors: per sample the share of the valid (gt != 0) pixels with
    |gt - depth| <= thresh * |gt|, averaged over the batch (NaN for a batch with a sample without a valid pixel, as
    the loss).  Not differentiable."""
    thresh = float(thresh)
    if math.isnan(thresh) or thresh < 0.0:
        raise ValueError("depth_accuracy: thresh >= 0 expected, got %r" % (thresh,))
    with torch.no_grad():
        if _on_hip(gt, initial, refined):
            acc_0, acc_1 = masked_mae(gt, initial, refined, thresh)[2:4]
        else:
            valid = torch.ne(gt, 0)
            lim = thresh * torch.abs(gt)
            p_valid = valid.sum((1, 2, 3)).to(gt.dtype)
            acc_0 = (valid & (torch.abs(gt - initial) <= lim)).sum((1, 2, 3)).to(gt.dtype).div(p_valid)
            acc_1 = (valid & (torch.abs(gt - refined) <= lim)).sum((1, 2, 3)).to(gt.dtype).div(p_valid)
        return acc_0.mean(), acc_1.mean()
