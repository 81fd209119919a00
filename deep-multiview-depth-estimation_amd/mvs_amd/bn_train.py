"""A train-mode BatchNorm + ReLU site of the regulariser under autograd on the HIP kernels
(CostVolumeReg.forward_live_train with MVS_TRAIN_BN=hip): out = relu(BN(z[box])), the batch statistics over all of
z plus the closed-form border term, as ONE autograd node.

  forward   ops.channel_stats (z read once, float64 slot sums), bn_sums._bn_train on the sums (the running
            statistics' update included), ops.bn_relu_ (the box read once, the output written once).  Saved: z and
            per-channel vectors, no other full-size tensor.
  backward  two passes of csrc/bn_train_bwd.hip around a per-channel closed form:
              ga = gy under the forward's ReLU mask (0 outside the box); S_g = sum ga, S_gz = sum ga z (float64)
              g_shift = S_g                g_scale = S_gz - mean S_g          g_mean = -scale S_g
              inv = (var + eps)^-1/2       g_weight = g_scale inv             g_bias = g_shift
              g_var = -1/2 weight inv^3 g_scale  (0 where the variance clamp was active)
              g_s2 = g_var / count         g_s1 = (g_mean - 2 mean g_var) / count         (g_c1, g_c2) = (g_s1, g_s2)
              gz = ga scale + g_s1 + 2 z g_s2 over ALL of z, written once in z's memory layout
            z and gy are read twice each; no atomics, nothing zeroed, no host synchronisation.
The torch path this replaces (bn_sums._sums / _apply_bn / ReLU / regions._crop_pad) moves the tensor through HBM ten
to twenty times per site and keeps three or four full-size intermediates alive until the backward.

The node also returns (scale, shift, mean) as differentiable per-channel outputs: bn_sums._bn_constant of them
(relu(BN(0)), the next layer's border term) carries its gradient back through the same closed form."""
import torch

from .bn_sums import _bn_train
from .train_switches import device_fp32, is_


def enabled(x):
    """MVS_TRAIN_BN=hip (train_switches.TABLE), for an fp32 device tensor under autograd."""
    return is_("MVS_TRAIN_BN", "hip") and device_fp32(x, grad=True)


def _memory(t):
    """(the contiguous memory of the logical NCDHW tensor t, channels_last): channels-last memory behind an NCDHW
    view is taken as it is ([B, d, h, w, C]), anything else as contiguous NCDHW."""
    if not t.is_contiguous() and t.permute(0, 2, 3, 4, 1).is_contiguous():
        return t.permute(0, 2, 3, 4, 1), True
    return t.contiguous(), False


def _logical(m, channels_last):
    return m.permute(0, 4, 1, 2, 3) if channels_last else m


def _crop(m, channels_last, box):
    """A contiguous COPY of the box (a whole-extent box too: bn_relu_ then works in place on it, never on z)."""
    sl = tuple(slice(lo, hi + 1) for lo, hi in box)
    view = m[(slice(None),) + sl] if channels_last else m[(slice(None), slice(None)) + sl]
    return view.clone(memory_format=torch.contiguous_format)


class _BnReluTrain(torch.autograd.Function):
    """(out, scale, shift, mean) = f(z, weight, bias, c1, c2); bn (its eps, momentum and buffers), the box and the
    count ride along.  c1 / c2: the float64 border term added to the sums, or None."""

    @staticmethod
    def forward(ctx, z, weight, bias, c1, c2, bn, box, count):
        from . import ops
        zm, cl = _memory(z)
        s1, s2 = ops.channel_stats(zm, cl)
        if c1 is not None:
            s1, s2 = s1 + c1, s2 + c2
        scale, shift, mean = _bn_train(bn, s1, s2, count)   # (bn.weight / bn.bias are weight / bias)
        if box is None:
            out = ops.bn_relu_(zm, cl, scale, shift, mean, out=torch.empty_like(zm))
        else:
            out = ops.bn_relu_(_crop(zm, cl, box), cl, scale, shift, mean)
        shift = shift.detach().clone()   # (_bn_train hands back bn.bias itself)
        ctx.save_for_backward(zm, weight, s1, s2, scale, shift, mean)
        ctx.geo = (cl, box, float(count), float(bn.eps), c1 is not None)
        return _logical(out, cl), scale, shift, mean

    @staticmethod
    def backward(ctx, gy, g_sc, g_sh, g_mu):
        from . import ops
        zm, weight, s1, s2, scale, shift, mean = ctx.saved_tensors
        cl, box, count, eps, has_extra = ctx.geo
        gym = gy.permute(0, 2, 3, 4, 1).contiguous() if cl else gy.contiguous()
        if gym.data_ptr() % 16:
            gym = gym.clone()
        s_g, s_gz = ops.bn_relu_bwd_reduce(zm, gym, cl, box, scale, shift, mean)
        # the closed form, float64 [C] device ops; mean / scale as the forward applied them (fp32 values)
        g_shift = s_g + g_sh.double()
        g_scale = s_gz - mean.double() * s_g + g_sc.double()
        g_mean = -scale.double() * s_g + g_mu.double()
        m = s1 / count
        var = s2 / count - m * m                      # _bn_train's variance before its clamp_min(0)
        inv = torch.rsqrt(var.clamp_min(0.0) + eps)
        g_var = torch.where(var >= 0.0, -0.5 * weight.double() * inv * inv * inv * g_scale, torch.zeros_like(var))
        g_s2 = g_var / count
        g_s1 = (g_mean - 2.0 * m * g_var) / count
        gz = None
        if ctx.needs_input_grad[0]:
            gz = _logical(ops.bn_relu_bwd_apply(zm, gym, cl, box, scale, shift, mean, g_s1, g_s2), cl)
        extra = (g_s1, g_s2) if has_extra else (None, None)
        return (gz, (g_scale * inv).to(weight.dtype), g_shift.to(weight.dtype)) + extra + (None, None, None)


def bn_relu_train(z, box, bn, extra, count):
    """relu(BN(z[box])) of the logical NCDHW tensor z (NCDHW-contiguous or channels-last memory) with bn in train
    mode: batch statistics from the sums over ALL of z (+ ``extra`` = (c1, c2), float64 [C], bn_sums.
    _border_class_sums' term, which may require grad) over ``count`` elements (it may exceed z's own count);
    bn's running statistics and num_batches_tracked are updated as bn_sums._bn_train does.  ``box``: None or an
    inclusive (lo, hi) index box per dim inside z's D, H, W extents.
    Returns (out, (scale, shift, mean)): out in z's memory layout; the three fp32 [C] vectors of
    BN(x) = (x - mean) * scale + shift are differentiable outputs of the same node (bn_sums._bn_constant of them
    carries gradient to bn's weight and bias, to z and to ``extra``); detach them where only their values are
    wanted."""
    if z.dim() != 5:
        raise ValueError("bn_relu_train expects [B, C, D, H, W], got %s" % (tuple(z.shape),))
    if box is not None:
        box = tuple((int(lo), int(hi)) for lo, hi in box)
        if len(box) != 3 or any(lo < 0 or hi < lo or hi >= d for (lo, hi), d in zip(box, z.shape[2:])):
            raise ValueError("box %s is not inside the extents %s" % (box, tuple(z.shape[2:])))
    c1, c2 = extra if extra is not None else (None, None)
    out, scale, shift, mean = _BnReluTrain.apply(z, bn.weight, bn.bias, c1, c2, bn, box, count)
    return out, (scale, shift, mean)
