"""The live-region regulariser's region convolutions under autograd (train.py:97-104 through
CostVolumeReg.forward_live_train's torch layers) with their FORWARD on the HIP region kernels
(csrc/conv3d_region.hip: fp32 MFMA, the eval path's kernels without the BN epilogue) and the per-tap-GEMM
backward (tap_gemm.conv3d_backward / conv_transpose3d_backward: the same box geometry as tap_gemm's
conv3d_box / conv_transpose3d_box).  The tap GEMMs accumulate every tap's product into the output in HBM
(27 read-modify-write passes over it); the region kernels keep the accumulators in registers.

  stride-2 conv_k_0 (model.py:101-107, stacked 32 -> 16 + 32 + 64 over R2)  mode S2, one launch per layer
  stride-1 conv_k_1 (model.py:108-113, on R1 from the padded R2 crop)         mode S1
  transposed deconv_3_0 / deconv_2_0 (model.py:117-120, the full box from M)  mode T2
MVS_TRAIN_REGION_FWD selects which (enabled()).  MVS_TRAIN_REGION_BWD (bwd_enabled(), default "taps") moves
the stride-1 layers' backward onto HIP kernels as well: the input gradient on the forward's region kernel
in its adjoint geometry, the weight gradient on csrc/conv3d_region_wgrad.hip.  MVS_TRAIN_S2_BWD
(s2_bwd_enabled(), default "taps") does the same for the stacked stride-2 layer: the input gradient on the
region kernel's transposed mode, the weight gradient on csrc/conv3d_s2_wgrad.hip, both from the NCDHW volume
in place.  MVS_TRAIN_T2_BWD (t2_bwd_enabled(), default "taps") does it for deconv_3_0 / deconv_2_0: the input
gradient on the region kernel's stride-2 mode with the channels-last output gradient as the volume, the weight
gradient on csrc/conv3d_t2_wgrad.hip.  deconv_1_0 (16 -> 8, the full-size output, dims=None in _tconv_region)
comes under none of these: MVS_TRAIN_DECONV1 (d1_enabled(), default "taps") moves it onto HIP kernels in both
directions at once -- the forward on csrc/deconv3d_region.hip in raw mode (one pass instead of 27 tap passes over
the output), the input and weight gradients on csrc/deconv3d_region_bwd.hip, reading the NCDHW output gradient in
place and x in the channels-last memory it arrives in."""
import os

import torch

from . import tap_gemm
from .regions import extent, origin

S2_SPLITS = (16, 32, 64)   # conv_1_0, conv_2_0, conv_3_0 output channels (the stacked S2 order)
S1_CHANNELS = (16, 32, 64)
T2_SHAPES = ((64, 32), (32, 16))   # (c_in, c_out) of deconv_3_0, deconv_2_0


def enabled(x, kind=None):
    """kind "s2" / "s1" / "t2"; MVS_TRAIN_REGION_FWD: a comma list of kinds (default "s1,t2"), "hip" (all)
    or "taps" (none).  The stride-2 forward stays on the tap GEMMs by default: with it on the HIP kernel
    test_gpu_train.py::test_train_mode_autograd_chain_smooth_loss's deconv_1_0 weight gradient lands 2.8x
    the CPU fp32 error from float64 (0.0074 against 0.0027)."""
    v = os.environ.get("MVS_TRAIN_REGION_FWD", "s1,t2")
    on = v == "hip" or (kind is not None and kind in v.split(","))
    return on and x.is_cuda and x.dtype == torch.float32 and torch.is_grad_enabled()


BWD_KINDS = ("s1",)               # kinds with a HIP backward
S1_BWD_CHANNELS = (16, 32, 64)    # channel counts of "s1" whose HIP backward beats the tap GEMMs


def bwd_enabled(kind, channels=None):
    """The backward of ``kind`` runs on the HIP kernels.  MVS_TRAIN_REGION_BWD, read on every call: a comma
    list of kinds, "hip" (every kind in BWD_KINDS) or "taps" (none: the per-tap GEMMs; the default)."""
    v = os.environ.get("MVS_TRAIN_REGION_BWD", "taps")
    on = kind in BWD_KINDS and (v == "hip" or kind in v.split(","))
    return on and (kind != "s1" or channels is None or channels in S1_BWD_CHANNELS)


def _region_w(w):      # Conv3d weight [co, ci, 3, 3, 3] -> [27][co][ci]
    return w.detach().permute(2, 3, 4, 0, 1).reshape(27, w.shape[0], w.shape[1]).contiguous()


def _region_wt(w):     # ConvTranspose3d weight [ci, co, 3, 3, 3] -> [27][co][ci]
    return w.detach().permute(2, 3, 4, 1, 0).reshape(27, w.shape[1], w.shape[0]).contiguous()


def _cf(t):            # channels-last [B, d, h, w, C] -> logical NCDHW view
    return t.permute(0, 4, 1, 2, 3)


def s2_bwd_enabled(x):
    """The backward of the stacked stride-2 layers (32 -> 16 + 32 + 64) runs on the HIP kernels
    (ops.conv3d_s2_region_wgrad / conv3d_s2_region_dgrad).  MVS_TRAIN_S2_BWD, read on every call: "hip", or
    "taps" (the per-tap GEMMs; the default).  A switch of its own: MVS_TRAIN_REGION_BWD never names "s2"."""
    on = os.environ.get("MVS_TRAIN_S2_BWD", "taps") == "hip"
    return on and x.is_cuda and x.dtype == torch.float32


class _S2Box(torch.autograd.Function):
    """The stride-2 convolution on its output box.  hip_fwd: the forward on the region kernel (one launch per
    layer), else tap_gemm.conv3d_box's arithmetic.  hip_bwd (the stacked 32 -> 112 layer only): the backward
    on ops.conv3d_s2_region_wgrad / conv3d_s2_region_dgrad, else tap_gemm.conv3d_backward.  Both are decided by
    the caller (s2_box: grad mode is off in here).  Only x and w are saved."""

    @staticmethod
    def forward(ctx, x, w, out_reg, pad, pad_lo, splits, hip_fwd, hip_bwd):
        size = extent(out_reg)
        if hip_fwd:
            from .ops import CONV_S2, conv3d_region
            n = list(x.shape[2:])
            org = origin(out_reg)
            xc = x.contiguous()
            ys, c0 = [], 0
            for co in splits:
                ys.append(conv3d_region(xc, None, _region_w(w[c0:c0 + co]), CONV_S2, n, org, size, None, None,
                                        list(pad)))
                c0 += co
            y = _cf(torch.cat(ys, -1) if len(ys) > 1 else ys[0])
        else:
            y = tap_gemm.conv3d_box(x, w, 2, tuple(pad_lo), tuple(size))
        ctx.save_for_backward(x, w)
        ctx.geo = (tuple(pad_lo), tuple(size))
        ctx.hip_bwd = hip_bwd
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        if not ctx.hip_bwd:
            gx, gw = tap_gemm.conv3d_backward(x, w, 2, ctx.geo[0], ctx.geo[1], gy, ctx.needs_input_grad[0],
                                              ctx.needs_input_grad[1])
            return gx, gw, None, None, None, None, None, None
        from . import ops
        gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv3d_s2_region_dgrad(gy_cl, w, tuple(x.shape[2:]), ctx.geo[0])
        if ctx.needs_input_grad[1]:
            gw = ops.conv3d_s2_region_wgrad(x, gy_cl, ctx.geo[0])
        return gx, gw, None, None, None, None, None, None


def _region_w_adjoint(w):   # Conv3d weight [co, ci, 3, 3, 3] -> the input gradient's [27][ci][co], taps flipped
    return w.detach().flip(2, 3, 4).permute(2, 3, 4, 1, 0).reshape(27, w.shape[1], w.shape[0]).contiguous()


class _S1Valid(torch.autograd.Function):
    """conv3d(xin, w) with padding 0 (xin: the zero-padded crop of _conv_s1_region).  With the HIP backward
    (bwd_enabled("s1", C)) the channels-last copy the forward makes anyway is what is saved, and the backward is
      d/dw  gw[co][ci][t] = sum gy[o][co] x[o + t][ci]                 ops.conv3d_region_wgrad
      d/dx  gx[i] = sum_t gy[i - t] w[.][.][t] = conv(gy, w~) on the box of xin, gy zero outside its own:
            the forward's region kernel with gy as the input region at origin 1 of a volume of xin's
            extent, w~[t][ci][co] = w[co][ci][2 - t] per dim."""

    @staticmethod
    def forward(ctx, xin, w):
        from .ops import CONV_S1, conv3d_region
        L = list(xin.shape[2:])
        out = [d - 2 for d in L]
        x_cl = xin.permute(0, 2, 3, 4, 1).contiguous()
        y = conv3d_region(x_cl, None, _region_w(w), CONV_S1, L, [1, 1, 1], out, [0, 0, 0], L, None)
        ctx.hip_bwd = bwd_enabled("s1", w.shape[0])
        ctx.save_for_backward(x_cl if ctx.hip_bwd else xin, w)
        ctx.out = tuple(out)
        return _cf(y)

    @staticmethod
    def backward(ctx, gy):
        xin, w = ctx.saved_tensors
        if not ctx.hip_bwd:
            return tap_gemm.conv3d_backward(xin, w, 1, 0, ctx.out, gy, ctx.needs_input_grad[0],
                                            ctx.needs_input_grad[1])
        from .ops import CONV_S1, conv3d_region, conv3d_region_wgrad
        gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            L = list(xin.shape[1:4])
            gx = _cf(conv3d_region(gy_cl, None, _region_w_adjoint(w), CONV_S1, L, [0, 0, 0], L, [1, 1, 1],
                                   list(ctx.out), None, per_lane=True))
        if ctx.needs_input_grad[1]:
            gw = conv3d_region_wgrad(xin, gy_cl)
        return gx, gw


def t2_bwd_enabled(x):
    """The backward of the transposed region convolutions deconv_3_0 / deconv_2_0 (T2_SHAPES) runs on the HIP
    kernels (ops.conv3d_t2_region_wgrad / conv3d_t2_region_dgrad).  MVS_TRAIN_T2_BWD, read on every call: "hip",
    or "taps" (the per-tap GEMMs; the default).  A switch of its own: MVS_TRAIN_REGION_BWD never names "t2"."""
    on = os.environ.get("MVS_TRAIN_T2_BWD", "taps") == "hip"
    return on and x.is_cuda and x.dtype == torch.float32


class _T2Box(torch.autograd.Function):
    """The transposed convolution on its output box, forward on the region kernel.  hip_bwd (decided by the
    caller, t2_box: T2_SHAPES under MVS_TRAIN_T2_BWD=hip): the backward on ops.conv3d_t2_region_wgrad /
    conv3d_t2_region_dgrad, reading gy in the channels-last memory autograd delivers it in and returning gx
    channels-last like x; else tap_gemm.conv_transpose3d_backward.  Only x and w are saved."""

    @staticmethod
    def forward(ctx, x, w, x_reg, out_reg, pad, dims, crop, hip_bwd=False):
        from .ops import CONV_T2, conv3d_region
        size = extent(out_reg)
        y = conv3d_region(x.permute(0, 2, 3, 4, 1).contiguous(), None, _region_wt(w), CONV_T2, list(dims),
                          origin(out_reg), size, origin(x_reg), extent(x_reg), list(pad))
        ctx.save_for_backward(x, w)
        ctx.geo = (tuple(crop), tuple(size))
        ctx.hip_bwd = hip_bwd
        return _cf(y)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        if not ctx.hip_bwd:
            gx, gw = tap_gemm.conv_transpose3d_backward(x, w, 2, ctx.geo[0], ctx.geo[1], gy, ctx.needs_input_grad[0],
                                                        ctx.needs_input_grad[1])
            return gx, gw, None, None, None, None, None, None
        from . import ops
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.conv3d_t2_region_dgrad(gy, w, tuple(x.shape[2:]), ctx.geo[0])
        if ctx.needs_input_grad[1]:
            gw = ops.conv3d_t2_region_wgrad(x, gy, ctx.geo[0])
        return gx, gw, None, None, None, None, None, None


D1_SHAPE = (16, 8)   # (c_in, c_out) of deconv_1_0


def d1_enabled(x):
    """deconv_1_0 (D1_SHAPE, the transposed layer whose output is the full-size volume) runs forward and backward
    on the HIP kernels under autograd (ops.deconv3d_k3s2 / deconv3d_k3s2_wgrad / deconv3d_k3s2_dgrad).
    MVS_TRAIN_DECONV1, read on every call: "hip", or "taps" (the per-tap GEMMs; the default, also when unset or
    empty).  A switch of its own: no other switch enables it and it enables nothing else."""
    on = os.environ.get("MVS_TRAIN_DECONV1", "taps") == "hip"
    return on and x.is_cuda and x.dtype == torch.float32


class _D1Box(torch.autograd.Function):
    """deconv_1_0 on its output box: the forward on csrc/deconv3d_region.hip in raw mode (no BN, no residual; one
    pass, y NCDHW), the backward on csrc/deconv3d_region_bwd.hip, reading gy NCDHW in place and returning gx in
    x's layout (channels-last memory at the training shapes).  The kernel's geometry is origin and padding with
    pad - 2 * origin = crop per dim: origin 0 and pad = crop is the same launch.  Only x and w are saved."""

    @staticmethod
    def forward(ctx, x, w, crop, size, cl):
        from . import ops
        y = ops.deconv3d_k3s2(x.permute(0, 2, 3, 4, 1) if cl else x, [0, 0, 0], w, list(size), list(crop),
                              None, None, None, None, channels_last=cl)
        ctx.save_for_backward(x, w)
        ctx.crop, ctx.cl = tuple(crop), cl
        return y

    @staticmethod
    def backward(ctx, gy):
        from . import ops
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = ops.deconv3d_k3s2_dgrad(gy, w, tuple(x.shape[2:]), ctx.crop, channels_last=ctx.cl)
        if ctx.needs_input_grad[1]:
            gw = ops.deconv3d_k3s2_wgrad(x, gy, ctx.crop)
        return gx, gw, None, None, None


def d1_applies(x, w):
    """_tconv_region sends the layer to d1_box: the switch on, a GPU fp32 tensor under autograd, the (16, 8) weight."""
    return d1_enabled(x) and torch.is_grad_enabled() and tuple(w.shape) == D1_SHAPE + (3, 3, 3)


def d1_box(x, w, out_reg, crop):
    """deconv_1_0 under MVS_TRAIN_DECONV1=hip (d1_applies).  Which memory layout the kernels read x in (and return
    gx in) is decided here, before apply: channels-last in place when x's memory is, else NCDHW."""
    from .ops import _is_cl5
    return _D1Box.apply(x, w, tuple(crop), tuple(extent(out_reg)), _is_cl5(x))


def s2_box(x, w, out_reg, pad, pad_lo, splits):
    """Forward and backward kind are decided here, before apply.  _conv_s2_region comes here when either
    switch is on: the forward is the HIP kernel when MVS_TRAIN_REGION_FWD names "s2", and the tap GEMMs when
    only MVS_TRAIN_S2_BWD brought the layer here (a direct call with neither switch keeps the HIP forward)."""
    hip_bwd = s2_bwd_enabled(x) and x.shape[1] == 32 and tuple(splits) == S2_SPLITS
    return _S2Box.apply(x, w, out_reg, pad, pad_lo, splits, enabled(x, "s2") or not s2_bwd_enabled(x), hip_bwd)


def s1_valid(xin, w):
    return _S1Valid.apply(xin, w)


def t2_box(x, w, x_reg, out_reg, pad, dims, crop):
    """The backward kind is decided here, before apply (deconv_1_0, 16 -> 8 with dims=None, never comes here:
    it goes to d1_box under MVS_TRAIN_DECONV1=hip and to the tap GEMMs otherwise)."""
    hip_bwd = t2_bwd_enabled(x) and (w.shape[0], w.shape[1]) in T2_SHAPES
    return _T2Box.apply(x, w, x_reg, out_reg, pad, dims, crop, hip_bwd)
