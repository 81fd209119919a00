"""Drop-in ``MVSNet`` (reference ``scripts/model.py:155-207``) on the MI355X cost-volume path.

Module tree and ``state_dict`` keys are the reference's (93 entries: ``feature_encoder.model.N.*``,
``cost_volume_reg.{conv_*,deconv_*,BN_*}.*``, ``depthmap_refine.model.N.*``), so reference
checkpoints load unchanged, and ``forward`` has the reference signature:

    forward(nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views)
        -> (initial_depth_map [B,1,h,w], refined_depth_map [B,1,h,w])

What changes is the hot path: ``model.py:177-181`` (per-plane kornia warp loop + torch.cat growth
+ 6-D variance) becomes ONE fused HIP kernel (``costvolume.warp_and_assemble_cost_volume``) and
``model.py:187`` the HIP soft-argmin.  In fp32 no-grad inference the 2-D encoder / refinement
convolutions and the 3-D regulariser's layers run on hand-written HIP kernels too (direct 2-D convs
with fused BN + ReLU, MFMA region convs on the live regions; conv_0_0 and
conv_1_0 on split-fp16 matrix-core kernels fed by the fused kernel's split volume, §3.5, exact-fp32
kernels with ``MVS_SPLIT_F16=0``).  Under autograd the regulariser's Conv3d / ConvTranspose3d run as
per-tap rocBLAS GEMMs with their own backward (``tap_gemm.py``) and the 2-D layers as
the PyTorch-ROCm modules; other dtypes and the full-volume reference leg (``forward_full`` without
grad) use PyTorch-ROCm (MIOpen).  Like
the reference (``model.py:164-166``) the instance attribute
``parameters`` is a LIST of tensors (``train.py:160`` passes it to Adam); use
``named_parameters()`` / ``state_dict()`` for module-generic code.

The encoder, the refinement net and ``MVSNet`` live here; the regulariser is ``regulariser.py`` (with
``regions.py``, ``bn_sums.py`` and ``streams.py``), whose helpers stay importable from this module.
"""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import eval_switches, streams, train_switches
from .bn_sums import _bn_constant, _bn_train, _bn_train_hip, _border_class_sums, _border_tables_u  # noqa: F401
from .config import MVSConfig
from .costvolume import warp_and_assemble_cost_volume
from .depthmap import extract_depth_map
from .regions import (_conv_s1_region, _conv_s2_region, _crop_pad, _grow, _taps, _tconv_input_region,  # noqa: F401
                      _tconv_region)
from .regulariser import CostVolumeReg, _bn_eval, _hip_inference
from .streams import _LANE, _side_stream  # noqa: F401

# (in, out, kernel, stride, padding) of the 2-D feature encoder (model.py:35-59), base_filt 8,
# DIM_REDUCE 4 -> 8 / 16 / 32 channels; BN+ReLU follow every conv but the last.
_ENCODER = [(3, 8, 3, 1, 1), (8, 8, 3, 1, 1), (8, 16, 5, 2, 2), (16, 16, 3, 1, 1),
            (16, 16, 3, 1, 1), (16, 32, 5, 2, 2), (32, 32, 3, 1, 1), (32, 32, 3, 1, 1)]
# refinement net (model.py:134-145): 4 -> 32 -> 32 -> 32 -> 1
_REFINE = [(4, 32, 3, 1, 1), (32, 32, 3, 1, 1), (32, 32, 3, 1, 1), (32, 1, 3, 1, 1)]


def _conv_bn_relu_stack(spec, device):
    layers = []
    for n, (cin, cout, k, s, p) in enumerate(spec):
        layers.append(nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=False, device=device))
        if n + 1 < len(spec):
            layers += [nn.BatchNorm2d(cout, eps=1e-5, momentum=0.1, device=device), nn.ReLU()]
    return nn.Sequential(*layers)


def conv2d_bwd_mode():
    """MVS_TRAIN_CONV2D_BWD, read once per _run_stack call: "hip" (mvs_amd/conv2d_train.py) or "taps" (the per-tap
    GEMMs; the default, also when unset or empty); anything else raises (train_switches.TABLE)."""
    return train_switches.read("MVS_TRAIN_CONV2D_BWD")


def conv2d_train_backends():
    """(the Conv2d layers go through tap_gemm under autograd: MVS_TRAIN_CONV2D=taps, their forward on the HIP
    kernel: MVS_TRAIN_CONV2D_FWD=hip), read once per _run_stack call."""
    return train_switches.is_("MVS_TRAIN_CONV2D", "taps"), train_switches.is_("MVS_TRAIN_CONV2D_FWD", "hip")


def _run_stack(seq, x, split_f16=False):
    """A conv -> BatchNorm -> ReLU stack (encoder / refinement).  In fp32 no-grad inference on the
    GPU the convolutions run on the direct HIP kernel (mvs::conv2d, csrc/conv2d_narrow.hip: exact fp32)
    with eval BN + ReLU fused into its epilogue; train-mode BN (test.py:61) takes one-pass float64
    batch sums of the convolution's output and one in-place BN + ReLU pass (csrc/channel_ops.hip),
    with the running statistics updated as torch does.  Elsewhere the modules themselves.
    ``split_f16`` (MVSConfig(arithmetic="split_f16"), opt-in): the 8..32-channel layers on the f16
    matrix cores with split operands (csrc/conv2d_split.hip)."""
    taps, hip_fwd = conv2d_train_backends() if _taps(x) else (False, False)
    if taps:
        # under autograd on a HIP device (train.py:97-104): the convolutions as per-tap rocBLAS GEMMs
        # (tap_gemm.conv2d), not MIOpen's (its first training step compiles its kernels: ~40 s at cfg 2)
        from . import tap_gemm
        from .ops import conv2d_supported
        # MVS_TRAIN_CONV2D_BWD=hip: both gradients on csrc/conv2d_bwd.hip too (conv2d_train.py; imported only then)
        hip_bwd = None
        if hip_fwd and conv2d_bwd_mode() == "hip":
            from . import conv2d_train as hip_bwd
        for layer in seq:
            if isinstance(layer, nn.Conv2d) and hip_fwd and conv2d_supported(layer) and x.dim() == 4:
                if hip_bwd is not None and hip_bwd.applies(layer, x):
                    x = hip_bwd.conv2d_hip(x, layer)    # the HIP forward kernel, HIP input and weight gradients
                    continue
                x = tap_gemm.conv2d_hip_fwd(x, layer)   # the HIP forward kernel, per-tap-GEMM backward
            elif isinstance(layer, nn.Conv2d) and tap_gemm.conv2d_applies(layer):
                x = tap_gemm.conv2d(x, layer.weight, layer.stride, layer.padding)
            else:
                x = layer(x)
        return x
    if not _hip_inference(x):
        return seq(x)
    from .ops import (CONV2D_SPLIT_SHAPES, bn_relu_, bound_words, channel_stats, conv2d, conv2d_split,
                      conv2d_supported)
    layers = list(seq)
    # split-fp16 MFMA convolutions (csrc/conv2d_split.hip) for the 8..32-channel inputs: every layer's
    # output carries bound words (one zeroed set per layer, one memset) that scale the next layer's input
    words = bound_words(len(layers), x.device) if split_f16 and eval_switches.conv2d_f16() else None

    def conv(layer, x, xb, yb, bn=None):
        """(y, whether yb now bounds y): the HIP convolutions for the reference's layer shapes"""
        if isinstance(layer, nn.Conv2d) and conv2d_supported(layer):
            k = layer.kernel_size[0]
            if xb is not None and (layer.in_channels, layer.out_channels, k, layer.stride[0]) in CONV2D_SPLIT_SHAPES:
                return conv2d_split(x, layer.weight, layer.stride[0], xb, yb, *(bn or ())), yb is not None
            return conv2d(x, layer.weight, layer.stride[0], *(bn or ()), y_bound=yb), yb is not None
        y = layer(x)
        if bn is None:
            return y, False
        return bn_relu_(y.contiguous(), False, *bn, y_bound=yb), yb is not None

    xb = None   # x's bound words (None: unknown)
    i = 0
    while i < len(layers):
        layer = layers[i]
        yb = None if words is None or not isinstance(layer, nn.Conv2d) else words[i]
        if (i + 2 < len(layers) and isinstance(layers[i + 1], nn.BatchNorm2d)
                and isinstance(layers[i + 2], nn.ReLU)):
            bn = layers[i + 1]
            if bn.running_mean is None or not bn.affine:   # no running statistics: the module
                return _run_tail(layers[i:], x)
            if bn.training:
                y = conv(layer, x, xb, None)[0].contiguous()
                x = bn_relu_(y, False, *_bn_train_hip(bn, *channel_stats(y, False), y.numel() // y.shape[1]),
                             y_bound=yb)
                bounded = yb is not None
            else:   # eval BN + ReLU fused into the convolution's epilogue
                x, bounded = conv(layer, x, xb, yb, _bn_eval(bn))
            i += 3
        else:
            x, bounded = conv(layer, x, xb, yb)
            i += 1
        xb = yb if bounded else None
    return x


def _run_tail(layers, x):
    for layer in layers:
        x = layer(x)
    return x


class FeatureEncoder(nn.Module):
    """model.py:22-65 -- images [N,3,H,W] -> features [N,32,H/4,W/4]."""

    def __init__(self, in_ch=3, base_filt=8, device=None):
        super().__init__()
        if (in_ch, base_filt) != (3, 8):
            raise ValueError("the reference encoder is fixed at in_ch=3, base_filt=8")
        self.model = _conv_bn_relu_stack(_ENCODER, device)
        self.split_f16 = False   # MVSNet.set_arithmetic

    def forward(self, x):
        return _run_stack(self.model, x, self.split_f16)


_UNIFORM = {}


def _uniform_depths(d_min, d_int):
    """Every sample has the same (d_min, d_int) -- DTU's 425 / 2.5 for every camera, and d_int = 1 in
    train.py:95 / test.py:84.  Only then is a chunk of samples' forward the whole batch's: image i uses
    the depth planes of sample i mod B (homography.py:24-26, view-major tiling), which changes with the
    chunk's B unless all rows are equal.  A device tensor's answer is cached per storage and version (one
    device-to-host read per new tensor)."""
    out = True
    for t in (d_min, d_int):
        if t.numel() <= 1:
            continue
        if t.device.type == "cpu":
            out = out and bool((t == t.reshape(-1)[0]).all())
            continue
        key = (t.data_ptr(), t._version, tuple(t.shape), str(t.device))
        hit = _UNIFORM.get(key)
        if hit is None:
            if len(_UNIFORM) > 256:
                _UNIFORM.clear()
            hit = _UNIFORM[key] = bool((t == t.reshape(-1)[0]).all().item())
        out = out and hit
    return out


class DepthRefinement(nn.Module):
    """model.py:129-152 -- residual refinement of the normalised depth."""

    def __init__(self, in_ch=4, base_filt=32, device=None):
        super().__init__()
        if (in_ch, base_filt) != (4, 32):
            raise ValueError("the reference refinement net is fixed at in_ch=4, base_filt=32")
        self.model = _conv_bn_relu_stack(_REFINE, device)
        self.split_f16 = False   # MVSNet.set_arithmetic

    def forward(self, depth_and_input):
        return _run_stack(self.model, depth_and_input, self.split_f16) + depth_and_input[:, 0].unsqueeze(1)


def _select_images(images, idx):
    """images[idx] for the reference-view indices (homography.py:29-36 returns them as a CPU int64
    tensor 0, V, 2V, ...): a strided view when they form such a progression, since indexing a
    device tensor with a CPU index copies it to the device, and that pageable copy synchronises
    the host with every kernel queued before it (a bubble in each inference step)."""
    if idx.device.type == "cpu" and idx.dim() == 1 and idx.numel() > 0 and not idx.is_floating_point():
        n = idx.numel()
        first = int(idx[0])
        step = int(idx[1]) - first if n > 1 else 1
        if step > 0 and first >= 0 and torch.equal(idx, first + step * torch.arange(n, dtype=idx.dtype)) \
                and first + step * (n - 1) < images.shape[0]:
            return images[first:first + step * (n - 1) + 1:step]
    return images[idx.to(images.device)]


class MVSNet(nn.Module):
    """model.py:155-207 with the fused MI355X cost volume.  ``cfg`` replaces the reference's
    import-time globals (D_NUM, D_SCALE, FEAT_H/W, PAD/OUTPAD); the default equals them."""

    def __init__(self, cfg: MVSConfig = None, device=None):
        super().__init__()
        self.cfg = cfg if cfg is not None else MVSConfig()
        self.feature_encoder = FeatureEncoder(device=device)
        self.cost_volume_reg = CostVolumeReg(device=device, pad=self.cfg.pad, outpad=self.cfg.outpad)
        self.depthmap_refine = DepthRefinement(device=device)
        # reference quirk kept for train.py:160 (Adam(model.parameters, ...)), model.py:164-166
        self.parameters = (list(self.feature_encoder.parameters()) +
                           list(self.cost_volume_reg.parameters()) +
                           list(self.depthmap_refine.parameters()))
        self.set_arithmetic(self.cfg.arithmetic)
        # eval inference over B >= 2 samples: chunks of samples issued on their own streams (forward)
        # (measured slower at cfg 2: 6.32 against 5.87 ms per step with 2 chunks, gpurun_out r6f -- off)
        self.pipeline_chunks = eval_switches.pipeline_chunks()

    def set_arithmetic(self, arithmetic):
        """"fp32" (the reference's numerics: every HIP layer in exact fp32) or "split_f16" (opt-in: the
        encoder, refinement and regulariser convolutions on the f16 matrix cores with split-fp16
        operands, the cost volume stored as its fp16 hi / lo parts; narrower than fp32)."""
        from .config import ARITHMETICS
        if arithmetic not in ARITHMETICS:
            raise ValueError("arithmetic must be one of %s, got %r" % (ARITHMETICS, arithmetic))
        self.cfg.arithmetic = arithmetic
        split = arithmetic == "split_f16"
        for m in (self.feature_encoder, self.cost_volume_reg, self.depthmap_refine):
            m.split_f16 = split
        return self

    def forward(self, nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views):
        if self._pipeline_ok(nn_input, d_min, d_int, batch_size):
            return self._forward_pipelined(nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views)
        return self._forward_one(nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views)

    def _pipeline_ok(self, nn_input, d_min, d_int, batch_size):
        """The sample-pipelined eval forward applies: HIP fp32 inference with every module in eval mode
        (samples are then independent: eval BatchNorm is elementwise), at least two samples, and
        pipeline_chunks > 1 (MVS_PIPELINE_CHUNKS; 1 = off)."""
        k = self.pipeline_chunks
        return (k > 1 and int(batch_size) >= 2 and _hip_inference(nn_input) and not self.training
                and not any(m.training for m in self.modules())
                and all(t.numel() == 1 or t.shape[0] == int(batch_size) for t in (d_min, d_int))
                and _uniform_depths(d_min, d_int))

    def _forward_pipelined(self, nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views):
        """forward over the batch in ``pipeline_chunks`` chunks of samples, each issued on its own stream
        (lane): one chunk's encoder and cost volume (VALU / HBM-store bound) run beside another chunk's
        regulariser (matrix cores), instead of the whole batch's phases one after another.  Every kernel of
        the eval forward computes each sample independently, so the depth maps are bit-identical to the
        one-stream forward (tests/test_gpu_parity.py::test_pipelined_forward_is_bit_identical)."""
        B, V = int(batch_size), int(n_views)
        k = min(self.pipeline_chunks, B)
        cuts = [B * i // k for i in range(k + 1)]
        device = nn_input.device
        main = torch.cuda.current_stream(device)
        per = lambda t, b0, b1: t if t.numel() == 1 else t[b0:b1]
        outs = []
        for i in range(k):
            b0, b1 = cuts[i], cuts[i + 1]
            st = streams._lane_stream(device, i)
            st.wait_stream(main)
            _LANE[0] = i + 1
            try:
                with torch.cuda.stream(st):
                    outs.append((st,) + self._forward_one(
                        nn_input[b0 * V:b1 * V], K_batch[b0 * V:b1 * V], R_batch[b0 * V:b1 * V],
                        T_batch[b0 * V:b1 * V], per(d_min, b0, b1), per(d_int, b0, b1), b1 - b0, V))
            finally:
                _LANE[0] = 0
        for st, ini, ref in outs:
            main.wait_stream(st)
            ini.record_stream(main)
            ref.record_stream(main)
        return torch.cat([o[1] for o in outs]), torch.cat([o[2] for o in outs])

    def forward_with_confidence(self, nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views):
        """forward's arguments; (initial, refined, confidence): forward's two depth maps and the photometric
        confidence [B, 1, h, w] of the initial one (fusion.photometric_confidence: the probability mass of the four
        hypothesis planes around it), taken from the probability volume before it is dropped.  Always the
        one-stream forward (_forward_one), whatever pipeline_chunks says; HIP device tensors only."""
        return self._forward_one(nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views,
                                 with_confidence=True)

    def _forward_one(self, nn_input, K_batch, R_batch, T_batch, d_min, d_int, batch_size, n_views,
                     with_confidence=False):
        c = self.cfg
        device = nn_input.device
        feature_maps = self.feature_encoder(nn_input)
        bf16 = c.cv_dtype == "bfloat16"
        reg = self.cost_volume_reg
        # HIP inference on the live paths: the cost volume goes straight to the regulariser's kernels
        # in the channel-quad layout (ops.cost_volume_c4: the fused kernel's 16-byte store; with the
        # bf16 opt-in ops.cost_volume_c4_bf16, 8 bytes)
        quads = (_hip_inference(feature_maps) and 2 <= n_views <= 8
                 and feature_maps.shape[1] % 4 == 0
                 and (reg.live_ok((c.d_num,) + tuple(feature_maps.shape[2:]))
                      or reg.live_train_ok((c.d_num,) + tuple(feature_maps.shape[2:]))))
        # eval mode with the split-fp16 regulariser: the fused kernel writes the split cost volume
        # (and in train-mode BN, test.py:61, whose live path reads the split volume the same way)
        live_n = (c.d_num,) + tuple(feature_maps.shape[2:])
        split = (quads and not bf16 and reg.split_f16 and (reg.live_ok(live_n) or reg.live_train_ok(live_n))
                 and feature_maps.shape[1] == 32)
        # ... and with the opt-in fused head kernel (MVS_CV_HEAD=1), the volume is not formed here at
        # all: the regulariser forms it on chip inside conv_0_0 / conv_1_0.  Opt-in:
        # its gathering producers corrupt one item sporadically; the default path
        # materialises the split volume and runs both convolutions in one pass (ops.split_head)
        deferred = split and reg.live_ok(live_n) and (c.d_num % 2 == 0 and n_views in (2, 3)
                                                      and all(p % 2 == 1 for p in reg.pad)
                                                      and eval_switches.cv_head())
        cost_volume, d_batch, ref_views = warp_and_assemble_cost_volume(
            K_batch, R_batch, T_batch, d_min, d_int, feature_maps, batch_size, n_views,
            d_num=c.d_num, d_scale=c.d_scale,
            cv_dtype=torch.bfloat16 if bf16 else torch.float32, channel_quads=quads and not deferred,
            split=split, deferred=deferred)
        if bf16 and not quads:
            # opt-in: the volume is STORED in bf16 (rounded once); the regulariser
            # computes in fp32 from the rounded values, as the HIP channel-quad path does
            cost_volume = cost_volume.float()
        prob_volume = self.cost_volume_reg(cost_volume)
        initial_depth_map = extract_depth_map(prob_volume, d_batch, c.n_depth_est)
        if with_confidence:
            from .fusion import photometric_confidence
            confidence = photometric_confidence(prob_volume, initial_depth_map, d_batch)
            del prob_volume
            return (initial_depth_map, self.refine(nn_input, initial_depth_map, d_min, d_int, ref_views),
                    confidence)
        return initial_depth_map, self.refine(nn_input, initial_depth_map, d_min, d_int, ref_views)

    def refine(self, nn_input, initial_depth_map, d_min, d_int, ref_views):
        """model.py:189-205: normalise, concat the downsampled reference image, refine, rescale."""
        c = self.cfg
        device = initial_depth_map.device
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_img = F.interpolate(_select_images(nn_input, ref_views), (c.feat_h, c.feat_w), mode="bilinear")
        if (_hip_inference(initial_depth_map) and initial_depth_map.dim() == 4 and initial_depth_map.shape[1] == 1
                and tuple(ref_img.shape) == (initial_depth_map.shape[0], 3) + tuple(initial_depth_map.shape[2:])
                and all(t.numel() == 1 or tuple(t.shape) == (initial_depth_map.shape[0], 1, 1, 1)
                        for t in (d_min, d_int))   # per sample [B, 1, 1, 1] (data.py) or one value
                and eval_switches.refine_glue()):
            # the elementwise steps on either side of the refinement net as one HIP launch each
            # (ops.refine_input / refine_output: 9 launches -> 2, bit-equal to the sequence below)
            from .ops import refine_input, refine_output
            x = refine_input(initial_depth_map, d_min, d_int, c.d_num, c.d_scale, ref_img)
            return refine_output(_run_stack(self.depthmap_refine.model, x, self.depthmap_refine.split_f16), x,
                                 d_min, d_int, c.d_num, c.d_scale)
        d_trans = d_min.to(device)
        d_span = d_int.to(device).mul(c.d_num).mul(c.d_scale)
        norm_depth = torch.div(torch.subtract(initial_depth_map, d_trans), d_span)
        refined = self.depthmap_refine(torch.cat((norm_depth, ref_img), dim=1))
        return refined.mul(d_span).add(d_trans)
