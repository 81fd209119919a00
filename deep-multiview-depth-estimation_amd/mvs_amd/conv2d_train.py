"""The 2-D feature encoder's and refinement net's Conv2d layers under autograd (train.py:97-104 through
model._run_stack) with BOTH gradients on HIP kernels (csrc/conv2d_bwd.hip), behind MVS_TRAIN_CONV2D_BWD:

  forward   ops.conv2d                   csrc/conv2d_narrow.hip, exact fp32 (what tap_gemm.conv2d_hip_fwd runs)
  d/dx      mvs_train::conv2d_dgrad      a gather per input pixel, gy's halo staged in LDS; NCHW in, NCHW out
  d/dw      mvs_train::conv2d_wgrad      v_mfma_f32_16x16x4_f32 over the output pixels, persistent workgroups,
                                         one partial slot each, summed in slot order (bit-reproducible)

tap_gemm._Conv2dHipTaps.backward, which this replaces, makes a channels-last copy of gy and a parity-grid copy of
x and runs 9 or 25 rocBLAS GEMMs per gradient with 1 to 32 channels on the GEMM's narrow sides.  Here x, gy and the
weight are read in the memory the modules hold them in, and gx comes back NCHW-contiguous: the BatchNorm2d before
the layer keeps MIOpen's NCHW kernels.

The two ops live in the namespace ``mvs_train``, registered when this module is first imported (model._run_stack
imports it under the switch only): the ``mvs`` namespace is the drop-in surface and stays as it is.

MVS_TRAIN_CONV2D_BWD (train_switches.TABLE; read by model.conv2d_bwd_mode once per _run_stack call): "hip", or "taps" (the
per-tap GEMMs; the default, also when unset or empty); anything else raises.  A switch of its own: no other switch
enables it and it enables nothing else.  It acts only where tap_gemm.conv2d_hip_fwd acts (MVS_TRAIN_CONV2D=taps,
MVS_TRAIN_CONV2D_FWD=hip, ops.conv2d_supported(layer), a 4-D fp32 HIP input), and only for the shapes in
CONV2D_BWD_SHAPES."""
import ctypes

import torch

from . import _lib
from .ops import CONV2D_SHAPES, _conv2d_out, _require_gpu

_F32 = torch.float32

# (c_in, c_out, k, stride) whose HIP backward beats the per-tap GEMMs by more than the runs' spread at the cfg-2
# sizes (tools/train_layer_ab.py --family conv2d, profiles/conv2d_bwd_layers_cfg2.txt); any other shape stays
# on the GEMMs under "hip" too
CONV2D_BWD_SHAPES = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1),
                     (4, 32, 3, 1), (32, 1, 3, 1))


def layer_shape(conv):
    return (conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0])


def applies(conv, x):
    """model._run_stack sends the layer here: a shape in CONV2D_BWD_SHAPES, a 4-D fp32 HIP input.  (The caller has
    established MVS_TRAIN_CONV2D=taps, MVS_TRAIN_CONV2D_FWD=hip, MVS_TRAIN_CONV2D_BWD=hip and ops.conv2d_supported.)"""
    return layer_shape(conv) in CONV2D_BWD_SHAPES and x.dim() == 4 and x.is_cuda and x.dtype == _F32


def _geometry(x_shape, w_shape, stride, gy_shape, what):
    """(n, c_in, c_out, h, w, k) of an NCHW input and a [c_out, c_in, k, k] weight whose output has gy_shape."""
    if len(x_shape) != 4 or len(w_shape) != 4 or w_shape[2] != w_shape[3] or w_shape[1] != x_shape[1]:
        raise ValueError("%s: x [n, c_in, h, w] and weight [c_out, c_in, k, k] expected, got %s and %s"
                         % (what, tuple(x_shape), tuple(w_shape)))
    n, cin, h, wd = x_shape
    cout, k = w_shape[0], w_shape[2]
    if (cin, cout, k, stride) not in CONV2D_SHAPES:
        raise ValueError("%s: unsupported (c_in, c_out, k, stride) %s" % (what, (cin, cout, k, stride)))
    want = (n, cout, _conv2d_out(h, k, stride), _conv2d_out(wd, k, stride))
    if tuple(gy_shape) != want:
        raise ValueError("%s: gy %s expected, got %s" % (what, want, tuple(gy_shape)))
    return n, cin, cout, h, wd, k


def wgrad_plan(n, c_in, c_out, h, w, k, stride):
    """(tiles, slots) of mvs_conv2d_wgrad for these dimensions (mvs_conv2d_wgrad_plan); ValueError when refused."""
    tiles, slots = ctypes.c_int(0), ctypes.c_int(0)
    st = _lib.load().mvs_conv2d_wgrad_plan(n, c_in, c_out, h, w, k, stride, ctypes.byref(tiles), ctypes.byref(slots))
    if st != _lib.MVS_OK:
        raise ValueError("mvs_conv2d_wgrad_plan: %s (%d)" % (_lib.STATUS.get(st, "?"), st))
    return tiles.value, slots.value


def _aligned(t):
    """t contiguous fp32 with a 16-byte-aligned base (a copy only if it is not already)."""
    t = t.to(_F32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


@torch.library.custom_op("mvs_train::conv2d_dgrad", mutates_args=())
def conv2d_dgrad(gy: torch.Tensor, weight: torch.Tensor, stride: int, h: int, w: int) -> torch.Tensor:
    """Input gradient gx [n, c_in, h, w] (NCHW-contiguous, every element written) of conv2d(x, weight, stride,
    padding k // 2) from gy [n, c_out, ho, wo] and the module's weight [c_out, c_in, k, k] (mvs_conv2d_dgrad)."""
    _require_gpu(gy, "gy")
    lib = _lib.load()
    n, cin, cout, h, w, k = _geometry((gy.shape[0], weight.shape[1], h, w), weight.shape, stride, gy.shape,
                                      "conv2d_dgrad")
    gy = _aligned(gy)
    wt = _aligned(weight.detach().to(gy.device))
    gx = torch.empty((n, cin, h, w), device=gy.device, dtype=_F32)
    st = lib.mvs_conv2d_dgrad(_lib.ptr(gy), _lib.ptr(wt), n, cin, cout, h, w, k, stride, _lib.ptr(gx),
                              _lib.stream_handle(gy.device))
    _lib.check(st, "mvs_conv2d_dgrad")
    return gx


@conv2d_dgrad.register_fake
def _(gy, weight, stride, h, w):
    return gy.new_empty((gy.shape[0], weight.shape[1], h, w))


@torch.library.custom_op("mvs_train::conv2d_wgrad", mutates_args=())
def conv2d_wgrad(x: torch.Tensor, gy: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """Weight gradient dw [c_out, c_in, k, k] of conv2d(x, weight, stride, padding k // 2) from x [n, c_in, h, w]
    and gy [n, c_out, ho, wo], both NCHW (mvs_conv2d_wgrad: fp32 MFMA, bit-reproducible)."""
    return _wgrad(x, gy, k, stride, None)


@conv2d_wgrad.register_fake
def _(x, gy, k, stride):
    return x.new_empty((gy.shape[1], x.shape[1], k, k))


def _wgrad(x, gy, k, stride, workspace):
    """conv2d_wgrad's body; ``workspace``: None, or fp32 device memory of at least the query's size to use as the
    partial slots (the tests fill it first)."""
    _require_gpu(x, "x")
    _require_gpu(gy, "gy")
    lib = _lib.load()
    n, cin, cout, h, w, k = _geometry(x.shape, (gy.shape[1], x.shape[1], k, k), stride, gy.shape, "conv2d_wgrad")
    x, gy = _aligned(x), _aligned(gy)
    nbytes = lib.mvs_conv2d_wgrad_workspace_bytes(n, cin, cout, h, w, k, stride)
    if nbytes == 0:
        raise ValueError("conv2d_wgrad: x %s, gy %s: element counts below 2^31 expected"
                         % (tuple(x.shape), tuple(gy.shape)))
    if workspace is None:
        workspace = torch.empty(nbytes // 4, device=x.device, dtype=_F32)
    elif workspace.numel() * 4 < nbytes or workspace.dtype != _F32 or workspace.data_ptr() % 16:
        raise ValueError("conv2d_wgrad: a 16-byte-aligned fp32 workspace of %d bytes expected" % nbytes)
    dw = torch.empty((cout, cin, k, k), device=x.device, dtype=_F32)
    st = lib.mvs_conv2d_wgrad(_lib.ptr(x), _lib.ptr(gy), n, cin, cout, h, w, k, stride, _lib.ptr(dw),
                              _lib.ptr(workspace), _lib.stream_handle(x.device))
    _lib.check(st, "mvs_conv2d_wgrad")
    return dw


class _Conv2dHip(torch.autograd.Function):
    """conv2d with the HIP forward (ops.conv2d) and the HIP gradients.  Only x and w are saved; the input
    gradient is not launched when x needs none (the encoder's first layer: x is the image)."""

    @staticmethod
    def forward(ctx, x, w, stride):
        from . import ops
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return ops.conv2d(x.contiguous(), w, stride)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()   # any other layout: made NCHW once, for both kernels
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = conv2d_dgrad(gy, w, ctx.stride, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1]:
            gw = conv2d_wgrad(x, gy, w.shape[2], ctx.stride)
        return gx, gw, None


def conv2d_hip(x, m):
    """m(x) for an nn.Conv2d that applies(): differentiable in x and m.weight, both gradients on HIP kernels."""
    return _Conv2dHip.apply(x, m.weight, m.stride[0])
