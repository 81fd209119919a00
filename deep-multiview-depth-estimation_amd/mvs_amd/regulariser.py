"""The 3-D cost-volume regulariser (reference ``scripts/model.py:68-126``) and the dispatch that decides
which of its evaluations runs: the fused head, the eval-mode live regions on the HIP kernels or through
PyTorch's layers, train-mode BatchNorm from sums, the live regions under autograd, or the full volume."""
import torch
import torch.nn as nn

from . import config as cfg_mod
from . import eval_switches, streams
from .bn_sums import _apply_bn, _bn_constant, _bn_train, _bn_train_hip, _border_class_sums, _sums
from .regions import (_conv_s1_region, _conv_s2_region, _crop_cf, _crop_cl, _crop_pad, _grow, _tconv_region,
                      extent, live_regions, origin)
from .train_switches import device_fp32, is_


def _bn_eval(bn):
    """Eval BatchNorm as (scale, shift, mean): y = (x - mean) * scale + shift, scale = weight /
    sqrt(running_var + eps) (torch's batch_norm_inference order); the scale is cached per parameter
    state (ops.derived)."""
    from .ops import derived
    eps = bn.eps
    scale = derived(("bn_scale", eps), (bn.weight, bn.running_var), lambda wt, var: wt / torch.sqrt(var + eps))
    return scale, bn.bias, bn.running_mean


class CostVolumeReg(nn.Module):
    """model.py:68-126 -- 3-D regulariser + softmax over depth (dim 2).

    Four branches read the cost volume (conv_k_0, k = 0..3, 8/16/32/64 channels); the stride-2
    convs use padding dim//2+1 so every level stays at full resolution (config.py:20)."""

    def __init__(self, in_ch=32, base_filt=8, device=None, pad=None, outpad=None):
        super().__init__()
        pad = cfg_mod.PAD if pad is None else pad
        outpad = cfg_mod.OUTPAD if outpad is None else outpad
        f1, f2, f4, f8 = base_filt, 2 * base_filt, 4 * base_filt, 8 * base_filt
        c3 = lambda i, o, s, p: nn.Conv3d(i, o, 3, stride=s, padding=p, bias=False, device=device)
        d3 = lambda i, o: nn.ConvTranspose3d(i, o, 3, stride=2, padding=pad, output_padding=outpad,
                                             bias=False, device=device)
        self.conv_0_0 = c3(in_ch, f1, 1, 1)
        self.conv_1_0 = c3(in_ch, f2, 2, pad)
        self.conv_2_0 = c3(in_ch, f4, 2, pad)
        self.conv_3_0 = c3(in_ch, f8, 2, pad)
        self.conv_1_1 = c3(f2, f2, 1, 1)
        self.conv_2_1 = c3(f4, f4, 1, 1)
        self.conv_3_1 = c3(f8, f8, 1, 1)
        self.deconv_3_0 = d3(f8, f4)
        self.deconv_2_0 = d3(f4, f2)
        self.deconv_1_0 = d3(f2, f1)
        self.conv_out = c3(f1, 1, 1, 1)
        self.ReLU = nn.ReLU()
        self.BN_0 = nn.BatchNorm3d(f1, eps=1e-5, momentum=0.1, device=device)
        self.BN_1 = nn.BatchNorm3d(f2, eps=1e-5, momentum=0.1, device=device)
        self.BN_2 = nn.BatchNorm3d(f4, eps=1e-5, momentum=0.1, device=device)
        self.BN_3 = nn.BatchNorm3d(f8, eps=1e-5, momentum=0.1, device=device)
        self.Norm = nn.Softmax(2)
        self.pad, self.outpad = tuple(pad), tuple(outpad)
        # eval-mode live-region evaluation (see forward_live); False = always the full-volume path
        self.live_region = True
        # False (default, MVSConfig(arithmetic="fp32")): every HIP layer in exact fp32 (the depth-Winograd
        # VALU conv_0_0, fp32-MFMA region convs).  True (arithmetic="split_f16", opt-in, narrower than
        # fp32): the f16 matrix cores with split-fp16 operands (csrc/split.h) read the split cost volume
        self.split_f16 = False

    def forward(self, cv):
        """cv [B, C, D, H, W] (the reference's input), an ops.BoundCostVolume (the channel-quad layout
        [B, C/4, D, H, W, 4] fp32 or split int32 with its bound words, ops.cost_volume_c4_absmax /
        cost_volume_c4_split), the bf16 channel-quad volume of ops.cost_volume_c4_bf16 (opt-in), or a
        costvolume.DeferredCostVolume -- the volume's inputs, consumed where it is formed by the fused
        head kernel (forward_live_head) or materialised for any other path.  The HIP live paths read
        the channel-quad volumes in place; other paths get the reference layout in fp32."""
        from .costvolume import DeferredCostVolume
        from .ops import BoundCostVolume, unsplit_cost_volume
        if isinstance(cv, DeferredCostVolume):
            if self.head_ok(cv):
                return self.forward_live_head(cv)
            cv = cv.materialize()
        bound = None
        if isinstance(cv, BoundCostVolume):
            cv, bound = cv.data, cv.absmax
        elif cv.dim() == 6 and cv.dtype == torch.int32:
            raise ValueError("a split cost volume is meaningless without its bound words: pass "
                             "ops.BoundCostVolume(cv, absmax) (what warp_and_assemble_cost_volume returns)")
        if cv.dim() == 6:
            if self.live_ok(cv.shape[2:5]) and _hip_cv(cv):
                return self.forward_live(cv, bound)
            if (cv.dtype == torch.int32 and bound is not None and self.split_f16 and self.live_train_ok(cv.shape[2:5])
                    and _hip_cv(cv)):
                return self.forward_live_train(cv, bound)   # the split-fp16 train-mode path reads it as is
            if cv.dtype == torch.int32:   # the split cost volume: fp32 values back (to 2^-22) for other paths
                cv = unsplit_cost_volume(cv, bound)
            if self.live_train_ok(cv.shape[2:5]) and _hip_cv(cv):
                return self.forward_live_train(cv, bound)
            cv = cv.permute(0, 1, 5, 2, 3, 4).reshape((cv.shape[0], 4 * cv.shape[1]) + tuple(cv.shape[2:5])).float()
        if self.live_ok(cv.shape[2:]):
            return self.forward_live(cv)
        if self.live_train_ok(cv.shape[2:]):
            return self.forward_live_train(cv)
        if self.live_autograd_ok(cv):
            return self.forward_live_train(cv)   # (the torch layers: differentiable)
        return self.forward_full(cv)

    @property
    def _bns(self):
        return self.BN_0, self.BN_1, self.BN_2, self.BN_3

    def _bn_batch_stats_ready(self):
        """Every BN in train mode with running statistics and affine parameters: what train-mode BN
        from sums (bn_sums._bn_train) reads and updates."""
        return all(bn.training and bn.track_running_stats and bn.running_mean is not None and bn.affine
                   for bn in self._bns)

    def live_autograd_ok(self, cv):
        """forward_live_train under autograd (train.py:97-104: model.train(), loss.backward()): the
        live-region evaluation is the same function of the volume and the parameters as forward_full
        (structural zeros and per-class constants are exact identities, not approximations), so its
        autograd gradient is forward_full's -- with the region layers on their live regions only (cfg 2:
        the stride-2 convs and the deeper levels on 1/8 .. 1/512 of the volume).  On a HIP device in fp32,
        train-mode BN with running statistics, the module's padding derived from the volume extent;
        MVS_TRAIN_LIVE=0 keeps forward_full."""
        return (self.live_region and device_fp32(cv, grad=True)
                and cv.dim() == 5 and not torch.is_autocast_enabled()
                and not is_("MVS_TRAIN_LIVE", "0") and self._live_geometry_ok(tuple(cv.shape[2:]))
                and self._bn_batch_stats_ready())

    def head_ok(self, dcv):
        """The fused head kernel applies to this deferred cost volume: eval-mode live regions with the
        split-fp16 convolutions, fp32 HIP inference, C = 32, 2-3 views, D even and every stride-2
        padding odd (the kernel's window ownership), MVS_CV_HEAD=1 (opt-in)."""
        n = tuple(dcv.shape[2:])
        return (eval_switches.cv_head() and self.split_f16 and self.live_ok(n)
                and _hip_inference(dcv.feature_maps) and dcv.shape[1] == 32 and dcv.n_views in (2, 3)
                and n[0] % 2 == 0 and all(p % 2 == 1 for p in self.pad))

    def forward_live_head(self, dcv):
        """forward_live with the cost volume consumed where it is formed: one fused
        kernel (ops.cost_volume_head, csrc/cv_head.hip) forms the variance plane by plane on chip and
        applies conv_0_0 + BN_0 + ReLU (full volume) and conv_1_0 + BN_1 + ReLU (on halo(B)); the only
        part of the volume written is conv_2_0's input box (the stride-2 windows of halo(C2), which
        contain conv_3_0's), as the split cost volume.  The rest of the live evaluation is
        _forward_live_hip's."""
        n = tuple(dcv.shape[2:])
        _, B, C2, _ = live_regions(n, self.pad)
        h1, h2 = _grow(B, n, 1), _grow(C2, n, 1)
        lo = [max(2 * a - p, 0) for (a, _), p in zip(h2, self.pad)]
        hi = [min(2 * b - p + 2, d - 1) + 1 for (_, b), p, d in zip(h2, self.pad, n)]
        y0, y1, box = dcv.head(self.conv_0_0.weight, _bn_eval(self.BN_0), self.conv_1_0.weight,
                               _bn_eval(self.BN_1), self.pad, origin(h1), extent(h1), lo, hi)
        return self._forward_live_hip(box.data, n, True, box.absmax, head=(y0, y1), cv_box=box.box_region())

    def live_train_ok(self, n):
        """forward_live_train applies: every BN in train mode with running statistics (test.py:61's
        `model.train()` under `torch.no_grad()`), no autograd, the module's padding derived from n."""
        return (self.live_region and not torch.is_grad_enabled() and self._live_geometry_ok(n)
                and self._bn_batch_stats_ready())

    def live_ok(self, n):
        """forward_live applies (eval BN, live_region on, the module's padding derived from n)."""
        return self.live_region and not self._bn_uses_batch_stats() and self._live_geometry_ok(n)

    def _live_geometry_ok(self, n):
        """forward_live relies on every U-Net level having the cost volume's extent n, which holds
        when the module's padding is the one config.py:20-21 derives from n.  A module built for
        another D or resolution takes forward_full, which (like the reference) then fails with the
        shape mismatch at the level sums instead of returning wrongly indexed levels."""
        from .config import pad_outpad
        return (self.pad, self.outpad) == pad_outpad(*n)

    def _bn_uses_batch_stats(self):
        return any(bn.training or bn.running_mean is None for bn in self._bns)

    def forward_live(self, cv, bound=None):
        """Eval-mode regulariser evaluated only where its values reach the output.

        The stride-2 convs pad every dim by n//2 + 1 (config.py:20), so output j of conv_k_0 reads
        inputs 2j-P .. 2j-P+2 and is exactly 0 outside the middle half of each dim; the stride-2
        transposed convs likewise only READ the middle half of their input (an input i lands on
        outputs 2i-P .. 2i-P+2, off the [0, n) output range elsewhere).  Tracing the U-Net back
        from the full-size output: deconv_1_0 needs its input on B (middle half), deconv_2_0 needs
        its input on C2 (the middle of B), deconv_3_0 on C3 -- so level k's convs are evaluated on
        its region only (+1 halo for the 3x3x3 stride-1 conv), with exact zero padding at the
        tensor's borders.  Every output element is the same sum of the same products as in
        forward_full (only structurally-zero products and discarded outputs are skipped); sums may
        be ordered differently by MIOpen's kernels for the smaller shapes (fp32 rounding level).
        Eval-mode BatchNorm is elementwise, so it commutes with the restriction; train-mode BN
        (batch statistics over the whole volume, test.py:61) uses forward_full.
        """
        if _hip_cv(cv):
            # (a channel-quad cost volume, cv.dim() == 6, only comes here: see forward)
            return self._forward_live_hip(cv, tuple(cv.shape[2:5]), cv.dim() == 6, bound)
        return self.forward_live_torch(cv)

    def forward_live_torch(self, cv):
        """forward_live through PyTorch's convolutions (MIOpen on a HIP device) whatever the mode:
        the same live regions, an implementation independent of the HIP kernels (test reference)."""
        act = lambda bn, y: self.ReLU(bn(y))
        n = tuple(cv.shape[2:5])
        full, B, C2, C3 = live_regions(n, self.pad)
        # torch layers (CPU, autograd): the same regions through PyTorch's convolutions
        y0 = act(self.BN_0, self.conv_0_0(cv))
        # level 1 on B, level 2 on C2, level 3 on C3 (regions carry their origin in the volume)
        lv = []
        for conv_a, conv_b, bn, reg in ((self.conv_1_0, self.conv_1_1, self.BN_1, B),
                                        (self.conv_2_0, self.conv_2_1, self.BN_2, C2),
                                        (self.conv_3_0, self.conv_3_1, self.BN_3, C3)):
            halo = _grow(reg, n, 1)
            y = act(bn, _conv_s2_region(cv, conv_a.weight, halo, self.pad))
            lv.append(act(bn, _conv_s1_region(y, halo, conv_b.weight, reg, n)))
        y1, y2, y3 = lv
        y3 = act(self.BN_2, _tconv_region(y3, C3, self.deconv_3_0.weight, C2, self.pad))
        y2 = act(self.BN_1, _tconv_region(y3 + y2, C2, self.deconv_2_0.weight, B, self.pad))
        z = act(self.BN_0, _tconv_region(y2 + y1, B, self.deconv_1_0.weight, full, self.pad)) + y0
        return self.Norm(self.conv_out(z))

    def _forward_live_hip(self, cv, n, c4=False, bound=None, head=None, cv_box=(None, None)):
        """forward_live on the HIP kernels: conv_0_0 (csrc/conv3d_narrow.hip), every region conv
        and transposed conv on the fp32 MFMA with channels-last region tensors and the eval BN +
        ReLU fused (csrc/conv3d_region.hip), deconv_1_0 + BN_0 + ReLU + `+ y0` and the `y2 + y1`
        sum in one kernel (csrc/deconv3d_region.hip), conv_out (conv3d_narrow.hip).  ``n``: the
        volume's extent; ``c4``: cv is the channel-quad volume, read by conv_0_0 and the three
        stride-2 convs with 16-byte loads; ``bound``: its bound words (the split-fp16 kernels'
        scale).  ``head``: (y0, y1) from the fused head kernel (forward_live_head) -- conv_0_0's and
        conv_1_0's outputs; cv is then the split volume on conv_2_0's input box only, ``cv_box``
        (origin, size) that box."""
        from .ops import (CONV_S1, CONV_S2, CONV_T2, bound_words, conv3d_k3, conv3d_k3_split, conv3d_region,
                          conv3d_region_split, conv_head_fp32, conv_s2_split, deconv3d_k3s2, region_weight,
                          softmax_depth, split_head, timed_kernel)
        org, size = origin, extent
        _, B, C2, C3 = live_regions(n, self.pad)
        dims, pad = list(n), list(self.pad)

        # conv_0_0 (VALU-bound) runs on a side stream, concurrently with the region chain (MFMA /
        # memory-latency-bound) that does not need it until deconv_1_0.  (Round 3's fp32 kernels measured
        # no gain from levels 2-3 beside level 1: 6.21-6.25 against 6.18-6.22 ms per cfg-2 step,
        # profiles/r03e_reg_layers.log; the split-fp16 path below does gain from levels 1 and 3 on side streams)
        main = torch.cuda.current_stream(cv.device)
        # the split cost volume (int32, csrc/split.h) always goes to the split-fp16 kernels; an fp32
        # channel-quad volume does when split_f16 is on and it carries bound words
        split_cv = c4 and cv.dtype == torch.int32
        bound = bound if split_cv or (c4 and self.split_f16 and cv.dtype == torch.float32) else None
        if split_cv and bound is None:
            raise ValueError("split cost volume without its bound words")
        # the split-fp16 conv_0_0 (MFMA, LDS-staged) gains nothing beside the region chain: both compete
        # for the same CUs (cfg 2: 5.67 ms serialised against 5.78 ms on a side stream,
        # profiles/r03/r03u_reg_layers.log); the exact-fp32 VALU kernel overlaps the MFMA chain
        side = main if bound is not None else streams._side_stream(cv.device)
        # the split-fp16 eval path also runs the stride-1 and transposed region convolutions on the f16
        # matrix cores (ops.conv3d_region_split, csrc/conv3d_region_split.hip; MVS_REGION_SPLIT=0: the
        # fp32-MFMA kernels): every region tensor they read carries bound words, raised by the kernel
        # that writes it -- rows 0-2 conv_k_0's outputs, 3-5 conv_k_1's, 6 deconv_3_0's (one memset)
        bw = bound_words(7, cv.device) if split_cv and eval_switches.region_split() else None
        y1_bounded = False
        if head is None and split_cv and self._split_head_ok(cv, n):
            # conv_0_0 + BN_0 + ReLU and conv_1_0 + BN_1 + ReLU in one pass over the split volume
            # (ops.split_head, csrc/cv_head.hip PRESPLIT mode): bit-equal to the two kernels below
            h1 = _grow(B, n, 1)
            head = split_head(cv, bound, self.conv_0_0.weight, *_bn_eval(self.BN_0), self.conv_1_0.weight,
                              *_bn_eval(self.BN_1), pad, org(h1), size(h1), None if bw is None else bw[0])
            y1_bounded = bw is not None
        # the exact-fp32 head (ops.conv_head_fp32, csrc/conv3d_narrow.hip C1), opt-in (MVS_FP32_HEAD=1):
        # conv_1_0 on the fp32 matrix cores inside conv_0_0's VALU kernel, from the same LDS tiles, then
        # conv_1_1 behind it on the side stream.  Measured slower: the fused kernel 3.60 ms against
        # 1.88 + 1.15 ms for the two kernels alone, the cfg-2 step 6.6-6.7 against 5.8 ms (packed or single
        # fp32 FMAs, padded channel planes: 3.61-4.10 ms; gpurun_out r6i / r6j) -- the f32 MFMA does not
        # co-issue beside the packed-f32 VALU stream, it takes the same SIMD cycles
        y1_done = None
        if head is None and bound is None and self._fp32_head_ok(cv, c4, pad):
            h1 = _grow(B, n, 1)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                y0, y1a = conv_head_fp32(cv, self.conv_0_0.weight, *_bn_eval(self.BN_0), self.conv_1_0.weight,
                                         *_bn_eval(self.BN_1), pad, org(h1), size(h1))
                y1_done = conv3d_region(y1a, None, region_weight(self.conv_1_1), CONV_S1, dims, org(B), size(B),
                                        org(h1), size(h1), None, *_bn_eval(self.BN_1), out_ncdhw=True)
            cv.record_stream(side)
        elif head is not None:
            y0, y1_head = head
        else:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                if bound is not None:
                    y0 = conv3d_k3_split(cv, bound, self.conv_0_0.weight, *_bn_eval(self.BN_0))
                    bound.record_stream(side)
                else:
                    with timed_kernel("conv_0_0"):   # (bench.py's roofline kernel in fp32 arithmetic)
                        y0 = conv3d_k3(cv, self.conv_0_0.weight, *_bn_eval(self.BN_0), in_c4=c4, wino_z=True)
            cv.record_stream(side)

        def level(k, conv_a, conv_b, bn, reg):
            halo = _grow(reg, n, 1)
            ab = None if bw is None else bw[k]   # ya's bound words
            if head is not None and reg is B:
                ya = y1_head   # conv_1_0 + BN_1 + ReLU on halo(B), from the head kernel
                ab = ab if y1_bounded else None
            elif bound is not None and conv_a.weight.shape[0] == 16:
                # conv_1_0 reads the whole volume: LDS-staged split-fp16 kernel (csrc/conv3d_s2_split.hip)
                ya = conv_s2_split(cv, bound, conv_a.weight, dims, org(halo), size(halo), pad, *_bn_eval(bn))
                ab = None
            elif split_cv and bw is not None:
                # conv_2_0 / conv_3_0 on the split-fp16 matrix cores, straight from the split volume
                ya = conv3d_region_split(cv, None, region_weight(conv_a), CONV_S2, dims, org(halo), size(halo),
                                         cv_box[0], cv_box[1], pad, bound, None, ab, *_bn_eval(bn))
            else:
                ya = conv3d_region(cv, None, region_weight(conv_a), CONV_S2, dims, org(halo), size(halo), cv_box[0],
                                   cv_box[1], pad, *_bn_eval(bn), in_c4=c4, absmax=bound if split_cv else None,
                                   y_bound=ab)
            # -> (output, channels-last?).  Level 1's output only feeds deconv_1_0's input sum: channels-first
            # for its loads on the fp32 path; the split path keeps it channels-last (deconv_2_0's epilogue
            # adds it, coalesced)
            if ab is not None:
                return conv3d_region_split(ya, None, region_weight(conv_b), CONV_S1, dims, org(reg), size(reg),
                                           org(halo), size(halo), None, ab, None, bw[3 + k], *_bn_eval(bn),
                                           out_ncdhw=False), True
            return conv3d_region(ya, None, region_weight(conv_b), CONV_S1, dims, org(reg), size(reg),
                                 org(halo), size(halo), None, *_bn_eval(bn), out_ncdhw=reg is B), reg is not B
        # (the fp32 path: the region chain on a high-priority stream, or levels 1 and 3 on side streams beside
        # level 2 as below, measured 5.99-6.93 against 5.86-5.89 ms per cfg-2 step -- not kept, gpurun_out r6g)
        if bw is not None and head is not None:   # (the split-fp16 region chain behind a head kernel)
            # level 1's conv_1_1 (LDS-bound) on a side stream beside levels 2-3 (L2-bound per-lane convs):
            # cfg-2 eval step 3.89-4.00 -> 3.80-3.93 ms (same box; the round-5 A/B script that measured it
            # is no longer in the tree)
            s1 = streams._side_stream(cv.device, 1)
            s1.wait_stream(main)
            with torch.cuda.stream(s1):
                y1, y1_cl = level(0, self.conv_1_0, self.conv_1_1, self.BN_1, B)
            # level 3 on a second side stream beside level 2 (3.91-3.93 -> 3.84-3.88 ms, the same script)
            s3 = streams._side_stream(cv.device, 2)
            s3.wait_stream(main)
            with torch.cuda.stream(s3):
                y3 = level(2, self.conv_3_0, self.conv_3_1, self.BN_3, C3)[0]
            y2 = level(1, self.conv_2_0, self.conv_2_1, self.BN_2, C2)[0]
            main.wait_stream(s3)
            y3.record_stream(main)
            main.wait_stream(s1)
            y1.record_stream(main)
        else:
            if y1_done is not None:   # (level 1 ran behind the fp32 head on the side stream)
                y1, y1_cl = y1_done, False
            else:
                y1, y1_cl = level(0, self.conv_1_0, self.conv_1_1, self.BN_1, B)
            y2 = level(1, self.conv_2_0, self.conv_2_1, self.BN_2, C2)[0]
            y3 = level(2, self.conv_3_0, self.conv_3_1, self.BN_3, C3)[0]
        if bw is not None:
            # deconv_3_0 + BN_2 + ReLU, then `+ y2` (model.py:119) in its epilogue: deconv_2_0 reads one tensor
            y32 = conv3d_region_split(y3, None, region_weight(self.deconv_3_0), CONV_T2, dims, org(C2), size(C2),
                                      org(C3), size(C3), pad, bw[5], None, bw[6], *_bn_eval(self.BN_2), y_addend=y2)
            # and, when level 1 ran split (channels-last), deconv_2_0's epilogue forms model.py:121's y2 + y1:
            # deconv_1_0 reads one channels-last tensor (else deconv_1_0 adds the channels-first y1 on load)
            y2 = conv3d_region_split(y32, None, region_weight(self.deconv_2_0), CONV_T2, dims, org(B), size(B),
                                     org(C2), size(C2), pad, bw[6], None, None, *_bn_eval(self.BN_1),
                                     out_ncdhw=not y1_cl, y_addend=y1 if y1_cl else None)
            if y1_cl:
                y1 = None
        else:
            y3 = conv3d_region(y3, None, region_weight(self.deconv_3_0), CONV_T2, dims, org(C2), size(C2),
                               org(C3), size(C3), pad, *_bn_eval(self.BN_2))
            y2 = conv3d_region(y3, y2, region_weight(self.deconv_2_0), CONV_T2, dims, org(B), size(B), org(C2),
                               size(C2), pad, *_bn_eval(self.BN_1), out_ncdhw=True)
        if side != main:   # (a stream waiting on itself is an event + barrier packet: a 6 us bubble)
            main.wait_stream(side)
            y0.record_stream(main)
            if y1_done is not None:
                y1.record_stream(main)
        z = deconv3d_k3s2(y2, org(B), self.deconv_1_0.weight, dims, pad, *_bn_eval(self.BN_0), y0, x2=y1,
                          channels_last=bw is not None and y1_cl)
        return softmax_depth(conv3d_k3(z, self.conv_out.weight))

    def _fp32_head_ok(self, cv, c4, pad):
        """ops.conv_head_fp32 applies: the fp32 channel-quad volume of 32 channels, conv_1_0 32 -> 16,
        every stride-2 padding odd (the kernel's window ownership), MVS_FP32_HEAD=1 (opt-in: slower, above)."""
        return (eval_switches.fp32_head() and c4 and cv.dtype == torch.float32
                and cv.dim() == 6 and cv.shape[1] == 8 and tuple(self.conv_1_0.weight.shape[:2]) == (16, 32)
                and all(p % 2 == 1 for p in pad))

    def _split_head_ok(self, cv, n):
        """ops.split_head applies to this split volume: C = 32 (8 channel quads), D even and every
        stride-2 padding odd (the kernel's window ownership), MVS_SPLIT_HEAD not 0."""
        return (eval_switches.split_head() and cv.shape[1] == 8 and n[0] % 2 == 0
                and all(p % 2 == 1 for p in self.pad))

    def forward_live_train(self, cv, bound=None):
        """Train-mode-BatchNorm regulariser (test.py:53,61: `model.train()` under `no_grad`)
        evaluated on live regions, exactly.

        With batch statistics every BN normalises by the mean / variance over the WHOLE volume, so
        the full-size tensors matter through their sums -- but most of them are structurally
        constant (the eval-mode argument of forward_live, carried through BN):
          * conv_k_0 (stride 2, padding n//2+1) is exactly 0 outside its middle-half region M, so
            its BN statistics are the region's sums over the full element count, and
            relu(BN(conv_k_0)) is the per-channel constant a_k = relu(BN(0)) outside M;
          * conv_k_1 (3x3x3, padding 1) of that field is, outside M grown by 1 (R1), a constant per
            channel and volume-border class (which of its taps fall inside the volume): 27 classes
            with known voxel counts, so its statistics are the R1 region's sums plus
            count x value (and count x value^2) per class;
          * the stride-2 transposed convs read only the middle half M of their input (forward_live),
            so deconv_3_0 / deconv_2_0 / deconv_1_0 are computed from the M-region tensors; their
            statistics need the full output, computed here in full (it is not constant).
        Every BatchNorm updates its running statistics once per use, in the reference's order
        (BN_0, BN_1, BN_2, BN_3, BN_1, BN_2, BN_3, BN_2, BN_1, BN_0), as forward_full does."""
        act = lambda y, bn: self.ReLU(_apply_bn(y, *bn))
        n = tuple(cv.shape[2:5])
        full, M = live_regions(n, self.pad)[:2]   # (M: forward_live's B)
        R1, R2 = _grow(M, n, 1), _grow(M, n, 2)
        bsz = cv.shape[0]
        count = bsz * n[0] * n[1] * n[2]
        if _hip_cv(cv):
            return self._forward_live_train_hip(cv, n, full, M, R1, R2, count, bound)
        from . import bn_train
        fused = bn_train.enabled(cv)

        def site(z, bn, z_reg=None, box=None, extra=None, crop_first=True):
            """One BN + ReLU site: (relu(BN(z)) on ``box`` of z's region z_reg -- all of z when None --, the BN's
            (scale, shift, mean)); ``extra``: the border term added to the sums.  MVS_TRAIN_BN=hip: one autograd
            node on the HIP kernels (bn_train.bn_relu_train); else the torch ops, the BN applied to the crop
            (crop_first) or the crop taken from the BN's output."""
            if fused:
                rel = None if box is None else tuple((lo - zlo, hi - zlo) for (zlo, _), (lo, hi) in zip(z_reg, box))
                return bn_train.bn_relu_train(z, rel, bn, extra, count)
            s1, s2 = _sums(z)
            if extra is not None:
                s1, s2 = s1 + extra[0], s2 + extra[1]
            p = _bn_train(bn, s1, s2, count)
            if box is None:
                return act(z, p), p
            if crop_first:
                return act(_crop_pad(z, z_reg, box, n), p), p
            return _crop_pad(act(z, p), z_reg, box, n), p
        y0 = _narrow_conv(self.conv_0_0, cv)
        y0 = site(y0, self.BN_0)[0]
        stage = []
        convs_a = ((self.conv_1_0, self.BN_1), (self.conv_2_0, self.BN_2), (self.conv_3_0, self.BN_3))
        # the three stride-2 convs read the same volume over the same region R2: ONE convolution with their
        # output channels stacked (under autograd one input layout pass, one input gradient)
        zs = _conv_s2_region(cv, torch.cat([c.weight for c, _ in convs_a], 0), R2, self.pad,
                             splits=tuple(c.weight.shape[0] for c, _ in convs_a))   # 0 outside M
        zs = zs.split([c.weight.shape[0] for c, _ in convs_a], 1)
        for z, (conv_a, bn) in zip(zs, convs_a):
            y, p = site(z, bn)
            stage.append((y, _bn_constant(p)))                      # relu(BN(0)) outside M
        lv = []
        for (y, a), conv_b, bn in zip(stage, (self.conv_1_1, self.conv_2_1, self.conv_3_1),
                                      (self.BN_1, self.BN_2, self.BN_3)):
            z = _conv_s1_region(y, R2, conv_b.weight, R1, n)
            # (the torch ops apply the BN on R1 and crop; the fused node applies it on M: the same values)
            lv.append(site(z, bn, R1, M, _border_class_sums(conv_b.weight, a, R1, n, bsz), crop_first=False)[0])
        y1, y2, y3 = lv
        # (the full outputs for the statistics; BN + ReLU on M only, the next layer's input)
        z = _tconv_region(y3, M, self.deconv_3_0.weight, full, self.pad, n)
        y3 = site(z, self.BN_2, full, M)[0]
        z = _tconv_region(y3 + y2, M, self.deconv_2_0.weight, full, self.pad, n)
        y2 = site(z, self.BN_1, full, M)[0]
        z = _tconv_region(y2 + y1, M, self.deconv_1_0.weight, full, self.pad)
        z = site(z, self.BN_0)[0] + y0
        return self.Norm(_narrow_conv(self.conv_out, z))

    def _forward_live_train_hip(self, cv, n, full, M, R1, R2, count, bound=None):
        """forward_live_train on the HIP kernels: raw (BN-free) region convs on the fp32 MFMA
        (conv3d_region.hip), conv_0_0 / conv_out (conv3d_narrow.hip), deconv_1_0
        (deconv3d_region.hip); batch statistics as float64 sums of the raw outputs; BN + ReLU
        applied in place to the region tensors (channels-last).  The transposed convs run over
        the full output volume (their statistics) and keep the M-region part.  ``cv`` may be the
        channel-quad volume (conv_0_0 and the stride-2 convs read it with 16-byte loads)."""
        from .ops import (CONV_S1, CONV_S2, CONV_T2, bn_relu_, bound_words, channel_stats, conv3d_k3,
                          conv3d_k3_split, conv3d_region, conv3d_region_split_sums, conv_s2_split_multi_sums,
                          deconv3d_k3s2, region_weight, softmax_depth)
        c4 = cv.dim() == 6
        split_cv = cv.dtype == torch.int32   # the split volume (forward: only with split_f16 and its bound words)
        # with split_f16 the stride-1 and transposed convs run on the split-fp16 matrix cores
        # (conv3d_region_split): their inputs' bound words are raised by the BN + ReLU passes -- rows 0-2
        # the conv_k_1 inputs, 4-5 conv_2_1 / conv_3_1's outputs, 6 deconv_3_0's (raw: the transposed
        # convs fold the BN + ReLU into their staging)
        bw = bound_words(7, cv.device) if self.split_f16 and eval_switches.region_split() else None
        bwr = lambda k: None if bw is None else bw[k]
        org, size = origin, extent
        dims, pad, bsz = list(n), list(self.pad), cv.shape[0]
        # conv_0_0 and its batch statistics on a side stream, concurrently with the region chain
        main = torch.cuda.current_stream(cv.device)
        side = streams._side_stream(cv.device)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            if bound is not None and c4 and self.split_f16 and cv.shape[1] == 8:
                # (fp32 channel quads with their bound words, or the split volume itself)
                # the channel-quad volume with its bound words: conv_0_0 on the split-fp16 matrix cores
                # (fp32-level error; 4.4 -> ~1 ms at cfg 2), raw output for the batch sums
                y0 = conv3d_k3_split(cv, bound, self.conv_0_0.weight)
            else:
                y0 = conv3d_k3(cv, self.conv_0_0.weight, in_c4=c4, wino_z=True)
            p0 = _bn_train_hip(self.BN_0, *channel_stats(y0, False), count)
        cv.record_stream(side)
        stage = []
        if split_cv:
            # conv_1_0, conv_2_0, conv_3_0 read the same split volume over the same region R2: one launch
            # (ops.conv_s2_split_multi_sums), the volume's operands loaded once for all three, the batch
            # sums formed in its epilogue
            zs = conv_s2_split_multi_sums(cv, [region_weight(c) for c in (self.conv_1_0, self.conv_2_0,
                                                                          self.conv_3_0)],
                                          dims, org(R2), size(R2), pad, bound, y_bound=bwr(0))
        for k, (conv_a, bn) in enumerate(((self.conv_1_0, self.BN_1), (self.conv_2_0, self.BN_2),
                                          (self.conv_3_0, self.BN_3))):
            if split_cv:
                z, s1, s2 = zs[k]
            else:
                z = conv3d_region(cv, None, region_weight(conv_a), CONV_S2, dims, org(R2), size(R2), None, None,
                                  pad, in_c4=c4)
                s1, s2 = channel_stats(z, True)
            p = _bn_train_hip(bn, s1, s2, count)
            if split_cv and bw is not None and k < 2:
                # conv_1_1 / conv_2_1's LDS kernels apply relu(BN(.)) in their staging: z stays raw, its
                # bound the three outputs' (row 0)
                stage.append(((z, p), p))
            else:
                stage.append((bn_relu_(z, True, *p, y_bound=bwr(2 if split_cv else k)), p))
            # (p: relu(BN(0)) outside M)

        def level_b(k, y, pa, conv_b, bn):
            # level 1 only feeds deconv_1_0's input sum: channels-first for its loads
            cf = bn is self.BN_1
            if bw is not None:   # sums over R1 in the epilogue, only M stored (the next layers read M)
                if isinstance(y, tuple):   # (raw conv_k_0 output, its BN): folded into the staging
                    xin, xbn, xbw = y[0], y[1], bw[0]
                else:
                    xin, xbn, xbw = y, None, bw[2 if split_cv else k]
                z, s1, s2 = conv3d_region_split_sums(xin, None, region_weight(conv_b), CONV_S1, dims, org(R1),
                                                     size(R1), org(R2), size(R2), None, xbw, out_ncdhw=cf,
                                                     store_origin=org(M), store_size=size(M),
                                                     y_bound=None if cf else bw[3 + k], x_bn=xbn)
            else:
                z = conv3d_region(y, None, region_weight(conv_b), CONV_S1, dims, org(R1), size(R1), org(R2),
                                  size(R2), None, out_ncdhw=cf)
                s1, s2 = channel_stats(z, not cf)
                z = (_crop_cf if cf else _crop_cl)(z, R1, M)
            p = _bn_train_hip(bn, s1, s2, count, border=(conv_b.weight, R1, n, bsz, pa))
            if bw is not None and not cf:
                # conv_2_1 / conv_3_1: raw, with its BN -- the BN + ReLU (and deconv_3_0's, with the + y2 sum)
                # applied in the transposed convs' LDS staging instead of a pass over each tensor
                # (ops.conv3d_region_split_sums x_bn / x2_bn)
                return (z, p)
            return bn_relu_(z, not cf, *p)

        # with the split-fp16 region convs, conv_1_1 and conv_2_1 on two side streams beside conv_3_1
        # (independent until the transposed convs; each BN's running-statistic updates stay in order: the
        # stream waits for main before and main for it after): train-mode step 11.9 -> 11.7 ms (same box;
        # the round-5 A/B script that measured it is no longer in the tree)
        args = list(zip(stage, (self.conv_1_1, self.conv_2_1, self.conv_3_1), (self.BN_1, self.BN_2, self.BN_3)))
        lv = [None, None, None]
        used = []
        for k in (0, 1, 2):
            (y, pa), conv_b, bn = args[k]
            if bw is not None and k < 2:
                st = streams._side_stream(cv.device, 1 + k)
                st.wait_stream(main)
                with torch.cuda.stream(st):
                    lv[k] = level_b(k, y, pa, conv_b, bn)
                used.append((st, lv[k]))
            else:
                lv[k] = level_b(k, y, pa, conv_b, bn)
        for st, out in used:
            main.wait_stream(st)
            for t in (out if isinstance(out, tuple) else (out,)):
                t.record_stream(main)
        y1, y2, y3 = lv
        if bw is not None:
            # the transposed convs over the full output (their batch sums, formed in the epilogue), only
            # M stored: the next layer reads M
            (z3, p3), (z2, p2) = y3, y2
            z, s1, s2 = conv3d_region_split_sums(z3, None, region_weight(self.deconv_3_0), CONV_T2, dims, [0, 0, 0],
                                                 dims, org(M), size(M), pad, bw[5], y_bound=bw[6],
                                                 store_origin=org(M), store_size=size(M), x_bn=p3)
            p = _bn_train_hip(self.BN_2, s1, s2, count)
            # deconv_2_0 reads relu(BN_2(deconv_3_0)) + relu(BN_2(conv_2_1)) (model.py:119-120), both formed
            # in its staging from the raw tensors
            z, s1, s2 = conv3d_region_split_sums(z, z2, region_weight(self.deconv_2_0), CONV_T2, dims, [0, 0, 0],
                                                 dims, org(M), size(M), pad, bw[6], x2_bound=bw[4], out_ncdhw=True,
                                                 store_origin=org(M), store_size=size(M), x_bn=p, x2_bn=p2)
            p = _bn_train_hip(self.BN_1, s1, s2, count)
            # relu(BN_1(deconv_2_0)) + y1 (model.py:121) formed in the BN pass: y1 >= 0 (a ReLU output), so
            # relu((y1 - 0) * 1 + 0) is y1 exactly; deconv_1_0 then reads one tensor
            c1 = y1.shape[1]
            one, zero = torch.ones(c1, device=y1.device), torch.zeros(c1, device=y1.device)
            y2 = bn_relu_(z, False, *p, r=y1, r_bn=(one, zero, zero))
            y1 = z3 = z2 = None
        else:
            z = conv3d_region(y3, None, region_weight(self.deconv_3_0), CONV_T2, dims, [0, 0, 0], dims, org(M),
                              size(M), pad)
            p = _bn_train_hip(self.BN_2, *channel_stats(z, True), count)
            y3 = bn_relu_(_crop_cl(z, full, M), True, *p)
            del z
            z = conv3d_region(y3, y2, region_weight(self.deconv_2_0), CONV_T2, dims, [0, 0, 0], dims, org(M),
                              size(M), pad, out_ncdhw=True)
            p = _bn_train_hip(self.BN_1, *channel_stats(z, False), count)
            y2 = bn_relu_(_crop_cf(z, full, M), False, *p)
        del z
        z = deconv3d_k3s2(y2, org(M), self.deconv_1_0.weight, dims, pad, None, None, None, None, x2=y1)
        main.wait_stream(side)
        for t in (y0,) + tuple(p0):
            t.record_stream(main)
        p = _bn_train_hip(self.BN_0, *channel_stats(z, False), count)
        # relu(BN_0(deconv_1_0)) + relu(BN_0'(conv_0_0)) formed in conv_out's staging (one pass over the
        # full volume fewer)
        return softmax_depth(conv3d_k3(z, self.conv_out.weight, x2=y0, in_bn=torch.cat((p, p0))))

    def forward_full(self, cv):
        act = lambda bn, y: self.ReLU(bn(y))
        # the BN modules are shared between levels exactly as in model.py:101-121; the two narrow
        # full-resolution layers run on the HIP kernel in no-grad fp32 inference (_narrow_conv),
        # e.g. test.py:61's train-mode BatchNorm under no_grad; under autograd on a HIP device
        # (train.py:97-104) every convolution runs as per-tap rocBLAS GEMMs (tap_gemm.py: MIOpen's
        # backward solvers for these shapes take minutes per step)
        conv = _train_conv if cv.is_cuda and torch.is_grad_enabled() else (lambda m, x: m(x))
        y0 = act(self.BN_0, _narrow_conv(self.conv_0_0, cv))
        y1 = act(self.BN_1, conv(self.conv_1_0, cv))
        y2 = act(self.BN_2, conv(self.conv_2_0, cv))
        y3 = act(self.BN_3, conv(self.conv_3_0, cv))
        y1 = act(self.BN_1, conv(self.conv_1_1, y1))
        y2 = act(self.BN_2, conv(self.conv_2_1, y2))
        y3 = act(self.BN_3, conv(self.conv_3_1, y3))
        y3 = act(self.BN_2, conv(self.deconv_3_0, y3))
        y2 = act(self.BN_1, conv(self.deconv_2_0, y3 + y2))
        y1 = act(self.BN_0, conv(self.deconv_1_0, y2 + y1))
        return self.Norm(_narrow_conv(self.conv_out, y1 + y0))


def _hip_inference(x):
    """fp32 inference on a HIP device (no autograd, no autocast): the regulariser's hand-written
    full-resolution layers apply."""
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
            and not torch.is_autocast_enabled())


def _hip_cv(cv):
    """_hip_inference for the regulariser's input: also the bf16 channel-quad cost volume of the
    reduced-precision opt-in (its HIP layers widen it to fp32 on load) and the split cost volume
    (int32 elements of fp16 hi / lo parts, read by the split-fp16 kernels)."""
    return _hip_inference(cv) or (cv.is_cuda and cv.dim() == 6 and cv.dtype in (torch.bfloat16, torch.int32)
                                  and not torch.is_grad_enabled() and not torch.is_autocast_enabled())


def _narrow_conv(conv, x):
    """conv_0_0 (32 -> 8) / conv_out (8 -> 1) at full resolution: on a HIP device, in fp32 and
    without autograd, the hand-written kernel (mvs::conv3d_k3, csrc/conv3d_narrow.hip: MIOpen
    runs these narrow full-volume layers at a few TFLOP/s); under autograd on a HIP device the
    per-tap GEMMs (_train_conv); otherwise the module itself."""
    if _hip_inference(x):
        from .ops import conv3d_k3
        return conv3d_k3(x, conv.weight)
    if x.is_cuda and torch.is_grad_enabled():
        from . import narrow_train
        if narrow_train.applies(conv, x):   # HIP forward, input gradient and weight gradient
            return narrow_train.conv3d(conv, x)
        return _train_conv(conv, x)
    return conv(x)


def _train_conv(m, x):
    """A regulariser Conv3d / ConvTranspose3d under autograd on a HIP device: per-tap rocBLAS GEMMs
    with their own backward (tap_gemm.py) instead of MIOpen (fp32 in and out)."""
    from . import tap_gemm
    if x.dtype != torch.float32 or torch.is_autocast_enabled():
        return m(x)
    return tap_gemm.conv_module(m, x)
