"""The live-region regulariser's region convolutions under autograd (train.py:97-104 through
CostVolumeReg.forward_live_train's torch layers) with their FORWARD on the HIP region kernels
(csrc/conv3d_region.hip: fp32 MFMA, the eval path's kernels without the BN epilogue) and the per-tap-GEMM
backward (tap_gemm.conv3d_backward / conv_transpose3d_backward: the same box geometry as tap_gemm's
conv3d_box / conv_transpose3d_box).  The tap GEMMs accumulate every tap's product into the output in HBM
(27 read-modify-write passes over it); the region kernels keep the accumulators in registers.

  stride-2 conv_k_0 (model.py:101-107, stacked 32 -> 16 + 32 + 64 over R2)  mode S2, one launch per layer
  stride-1 conv_k_1 (model.py:108-113, on R1 from the padded R2 crop)         mode S1
  transposed deconv_3_0 / deconv_2_0 (model.py:117-120, the full box from M)  mode T2
Which layer runs where is decided once per layer by s2_route / s1_route / tconv_route below, from the training
switches (train_switches.TABLE lists them: what each moves, its words and its default)."""
import torch

from . import tap_gemm
from .regions import extent, origin
from .train_switches import device_fp32, is_, names

S2_SPLITS = (16, 32, 64)   # conv_1_0, conv_2_0, conv_3_0 output channels (the stacked S2 order)
S1_CHANNELS = (16, 32, 64)
T2_SHAPES = ((64, 32), (32, 16))   # (c_in, c_out) of deconv_3_0, deconv_2_0
D1_SHAPE = (16, 8)                 # (c_in, c_out) of deconv_1_0
BWD_KINDS = ("s1",)               # kinds with a HIP backward under MVS_TRAIN_REGION_BWD
S1_BWD_CHANNELS = (16, 32, 64)    # channel counts of "s1" whose HIP backward beats the tap GEMMs


# The switches as predicates (train_switches.TABLE documents each).

def enabled(x, kind=None):
    """The forward of ``kind`` ("s2" / "s1" / "t2") runs on the HIP region kernel: MVS_TRAIN_REGION_FWD."""
    return names("MVS_TRAIN_REGION_FWD", kind) and device_fp32(x, grad=True)


def bwd_enabled(kind, channels=None):
    """The backward of ``kind`` runs on the HIP kernels: MVS_TRAIN_REGION_BWD, for the kinds in BWD_KINDS."""
    on = kind in BWD_KINDS and names("MVS_TRAIN_REGION_BWD", kind)
    return on and (kind != "s1" or channels is None or channels in S1_BWD_CHANNELS)


def s2_bwd_enabled(x):
    """The stacked stride-2 layers' backward runs on ops.conv3d_s2_region_wgrad / _dgrad: MVS_TRAIN_S2_BWD."""
    return is_("MVS_TRAIN_S2_BWD", "hip") and device_fp32(x)


def t2_bwd_enabled(x):
    """deconv_3_0 / deconv_2_0's backward runs on ops.conv3d_t2_region_wgrad / _dgrad: MVS_TRAIN_T2_BWD."""
    return is_("MVS_TRAIN_T2_BWD", "hip") and device_fp32(x)


def d1_enabled(x):
    """deconv_1_0 runs forward and backward on ops.deconv3d_k3s2 / _wgrad / _dgrad: MVS_TRAIN_DECONV1."""
    return is_("MVS_TRAIN_DECONV1", "hip") and device_fp32(x)


def d1_applies(x, w):
    """d1_enabled for a tensor under autograd and the (16, 8) weight."""
    return d1_enabled(x) and torch.is_grad_enabled() and tuple(w.shape) == D1_SHAPE + (3, 3, 3)


# One routing decision per layer family, asked once by regions.py (inside its own "under autograd on a HIP device
# in fp32" branch): None = stay on the tap GEMMs, else the (HIP forward?, HIP backward?) pair the autograd box is
# applied with.

def s2_route(x, w, whole, splits, direct=False):
    """The stride-2 layer on its output box.  ``whole``: the box reads the whole volume (no crop); ``splits``: the
    output channels of the layers stacked in ``w``.  The layer goes to _S2Box when either MVS_TRAIN_REGION_FWD
    names "s2" or MVS_TRAIN_S2_BWD is "hip".  ``direct`` (s2_box called without a route, as tests do): no gate."""
    fwd, bwd = enabled(x, "s2"), s2_bwd_enabled(x)
    if not direct and not (whole and splits is not None and x.shape[1] == 32
                           and tuple(splits) in (S2_SPLITS, (16,), (32,), (64,)) and (fwd or bwd)):
        return None
    # the forward is the tap GEMMs' when only MVS_TRAIN_S2_BWD brought the layer here; with neither switch (a direct
    # call only) it stays the HIP kernel.  The HIP backward exists for the stacked (16, 32, 64) split of 32 input
    # channels only.
    return fwd or not bwd, bwd and x.shape[1] == 32 and tuple(splits) == S2_SPLITS


def s1_backward(w):
    """The HIP backward of a stride-1 layer: MVS_TRAIN_REGION_BWD names "s1" and c_out is in S1_BWD_CHANNELS."""
    return bwd_enabled("s1", w.shape[0])


def s1_route(x, w):
    """The stride-1 layer on its padded crop: the HIP forward (_S1Valid) for the square S1_CHANNELS weights when
    MVS_TRAIN_REGION_FWD names "s1"; the backward as s1_backward says."""
    if not (enabled(x, "s1") and w.shape[0] == w.shape[1] and w.shape[0] in S1_CHANNELS):
        return None
    return True, s1_backward(w)


def t2_backward(x, w):
    """The HIP backward of a transposed layer: MVS_TRAIN_T2_BWD=hip and a (c_in, c_out) in T2_SHAPES."""
    return t2_bwd_enabled(x) and (w.shape[0], w.shape[1]) in T2_SHAPES


def tconv_route(x, w, no_dims):
    """The transposed layers.  With the volume extent given (``no_dims`` False: deconv_3_0 / deconv_2_0) the HIP
    forward (_T2Box) for T2_SHAPES when MVS_TRAIN_REGION_FWD names "t2", the backward as t2_backward says.  Without
    it (deconv_1_0, whose output is the full-size volume) both directions on HIP (_D1Box) when d1_applies: D1_SHAPE
    under MVS_TRAIN_DECONV1=hip.  No other switch moves deconv_1_0, and MVS_TRAIN_DECONV1 moves nothing else."""
    if no_dims:
        return (True, True) if d1_applies(x, w) else None
    if enabled(x, "t2") and (w.shape[0], w.shape[1]) in T2_SHAPES:
        return True, t2_backward(x, w)
    return None


def _region_w(w):      # Conv3d weight [co, ci, 3, 3, 3] -> [27][co][ci]
    return w.detach().permute(2, 3, 4, 0, 1).reshape(27, w.shape[0], w.shape[1]).contiguous()


def _region_wt(w):     # ConvTranspose3d weight [ci, co, 3, 3, 3] -> [27][co][ci]
    return w.detach().permute(2, 3, 4, 1, 0).reshape(27, w.shape[1], w.shape[0]).contiguous()


def _cf(t):            # channels-last [B, d, h, w, C] -> logical NCDHW view
    return t.permute(0, 4, 1, 2, 3)


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
    (hip_bwd, decided by the caller) the channels-last copy the forward makes anyway is what is saved, and the backward is
      d/dw  gw[co][ci][t] = sum gy[o][co] x[o + t][ci]                 ops.conv3d_region_wgrad
      d/dx  gx[i] = sum_t gy[i - t] w[.][.][t] = conv(gy, w~) on the box of xin, gy zero outside its own:
            the forward's region kernel with gy as the input region at origin 1 of a volume of xin's
            extent, w~[t][ci][co] = w[co][ci][2 - t] per dim."""

    @staticmethod
    def forward(ctx, xin, w, hip_bwd):
        from .ops import CONV_S1, conv3d_region
        L = list(xin.shape[2:])
        out = [d - 2 for d in L]
        x_cl = xin.permute(0, 2, 3, 4, 1).contiguous()
        y = conv3d_region(x_cl, None, _region_w(w), CONV_S1, L, [1, 1, 1], out, [0, 0, 0], L, None)
        ctx.hip_bwd = hip_bwd
        ctx.save_for_backward(x_cl if ctx.hip_bwd else xin, w)
        ctx.out = tuple(out)
        return _cf(y)

    @staticmethod
    def backward(ctx, gy):
        xin, w = ctx.saved_tensors
        if not ctx.hip_bwd:
            return tap_gemm.conv3d_backward(xin, w, 1, 0, ctx.out, gy, ctx.needs_input_grad[0],
                                            ctx.needs_input_grad[1]) + (None,)
        from .ops import CONV_S1, conv3d_region, conv3d_region_wgrad
        gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            L = list(xin.shape[1:4])
            gx = _cf(conv3d_region(gy_cl, None, _region_w_adjoint(w), CONV_S1, L, [0, 0, 0], L, [1, 1, 1],
                                   list(ctx.out), None, per_lane=True))
        if ctx.needs_input_grad[1]:
            gw = conv3d_region_wgrad(xin, gy_cl)
        return gx, gw, None


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


# The boxes' entry points.  regions.py passes the route it asked for; a call without one (tests, tools) asks here.
# Either way the backends are fixed before apply (grad mode is off inside forward).

def d1_box(x, w, out_reg, crop):
    """deconv_1_0 where tconv_route sent it.  Which memory layout the kernels read x in (and return gx in) is
    decided here: channels-last in place when x's memory is, else NCDHW."""
    from .ops import _is_cl5
    return _D1Box.apply(x, w, tuple(crop), tuple(extent(out_reg)), _is_cl5(x))


def s2_box(x, w, out_reg, pad, pad_lo, splits, route=None):
    hip_fwd, hip_bwd = route or s2_route(x, w, True, splits, direct=True)
    return _S2Box.apply(x, w, out_reg, pad, pad_lo, splits, hip_fwd, hip_bwd)


def s1_valid(xin, w, route=None):
    return _S1Valid.apply(xin, w, route[1] if route else s1_backward(w))


def t2_box(x, w, x_reg, out_reg, pad, dims, crop, route=None):
    return _T2Box.apply(x, w, x_reg, out_reg, pad, dims, crop, route[1] if route else t2_backward(x, w))
