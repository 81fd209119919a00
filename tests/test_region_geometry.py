"""The forward region kernels and the live regulariser on the HIP path across volume shapes.

CostVolumeReg sends every eval-mode or train-mode-under-no_grad call on a HIP device through the region
kernels whenever its padding is the one derived from the volume; no guard looks at the volume's size,
parity or aspect.  The shapes below are those at which the region geometry degenerates:

    (1, 2, 3)     D = 1; every region is the volume; transposed-conv parity classes with zero rows
    (3, 1, 5)     h = 1
    (2, 3, 4)     mixed padding parity, every extent below one tile
    (5, 6, 6)     C2 = C3; halo(B) = the volume
    (7, 9, 11)    all odd, output padding 0
    (13, 10, 17)  test_region_deconv_fused_epilogue_matches_torch's shape, for every layer
    (9, 4, 33)    B is 17 wide (16 + 1); H below a tile
    (16, 5, 66)   D even but W padding even (no split head); B is 34 wide: three x-tiles
    (6, 18, 35)   all-even padding: every transposed-conv parity class and stride-2 window origin flipped
    (20, 32, 40)  several workgroups per launch; D even and padding odd: the split-head branch

Part 1 (test_region_layer): every call _forward_live_hip and _forward_live_train_hip make, one layer at
a time on the regions they form, against torch's convolution of the zero-extended tensors in float64 on
the CPU, with the acceptance criteria of test_region_conv_matches_torch (fp32 kernels),
test_region_split_conv_matches_torch (split-fp16 kernels), test_region_split_sums_and_store_box (batch
sums) and test_region_split_*_folded_input_bn (BN + ReLU folded into the staging): region_cases.check_*.
Batch sizes 1 and 3 alternate over geometries and layers.

Part 2 (test_live_chain): the whole chain against copy.deepcopy(model).double().forward_full on the CPU,
eval and train mode, fp32 and split-fp16 arithmetic, every input form CostVolumeReg.forward distinguishes,
batch 1 and 3.  Caps: fp32 eval rtol 1e-4 / atol 1e-7, train rtol 1e-4 / atol 1e-6, running statistics
rtol 1e-5 / atol 1e-6 (test_*live_regulariser_gpu_matches_full_volume); split-fp16 probabilities rtol 2e-3 /
atol 1e-7 (test_mvsnet_end_to_end's bound on the regulariser's output), its running statistics within 2x the
fp32 HIP chain's error on the same input + the fp32 tolerance.  Worst measured max relative probability
error over the nine geometries with D > 1, both batch sizes, every input form (the PARITY lines carry
each case):

    mode   arithmetic   measured   cap
    eval   fp32         4.9e-7     1e-4
    eval   split_f16    5.1e-7     2e-3
    train  fp32         2.3e-6     1e-4
    train  split_f16    2.2e-6     2e-3
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from region_cases import (GEOMETRIES, Regions, batch_of, bound_of, cf, check_fp32, check_split, check_sums, cl,
                          conv_w27, errs, gid, org, set_bound, size, sl, split_volume, tconv_w27, unsplit_ncdhw,
                          volume_bound_words, zero_ext)
from test_gpu_parity import _bn_params, _bn_relu, _to_c4

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def dev(*ts):
    out = tuple(None if t is None else t.to(DEV) for t in ts)
    return out[0] if len(out) == 1 else out


class Cx:
    """One (geometry, layer) case: the regions, the batch size and a seeded generator."""

    def __init__(self, n, k):
        self.n, self.r = tuple(n), Regions(n)
        self.b = batch_of(n, k)
        self.g = torch.Generator().manual_seed(1000 * k + 7 * n[0] + 3 * n[1] + n[2])
        self.dims, self.pad = list(n), list(self.r.pad)

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.g)

    def bn(self, c):
        return _bn_params(c, self.g)


def _s2_inputs(cx):
    """A cost-volume-like (non-negative) volume in its four forms: NCDHW, fp32 channel quads, the split
    volume with its bound words, and the values the split volume holds (NCDHW)."""
    x = cx.randn(cx.b, 32, *cx.n).square()
    words = volume_bound_words(x)
    sp = split_volume(_to_c4(x), words)
    return x, words, sp, unsplit_ncdhw(sp, words)


def _s2_eval(cx, cout, out_reg):
    """conv_k_0 + BN + ReLU from the full volume onto a halo region: conv3d_region from the NCDHW, the
    channel-quad and the split volume; conv3d_region_split from the split volume; for 32 -> 16 also
    conv_s2_split from the fp32 channel quads with their bound words and from the split volume."""
    from mvs_amd import ops
    r = cx.r
    x, words, sp, xs = _s2_inputs(cx)
    wt = cx.randn(cout, 32, 3, 3, 3) * 0.1
    bn = cx.bn(cout)
    f = lambda xx, ww: _bn_relu(F.conv3d(xx, ww, stride=2, padding=r.pad), *(t.to(xx.dtype) for t in bn))[sl(out_reg)]
    ref, reft = f(x.double(), wt.double()), f(x, wt)
    refs, refts = f(xs.double(), wt.double()), f(xs, wt)
    w27, wd, bnd, wordsd, spd = dev(conv_w27(wt)), dev(wt), dev(*bn), dev(words), dev(sp)
    geo = (ops.CONV_S2, cx.dims, org(out_reg), size(out_reg), None, None, cx.pad)
    bw = ops.bound_words(3, DEV)
    with torch.no_grad():
        ya = ops.conv3d_region(dev(x), None, w27, *geo, *bnd)
        yb = ops.conv3d_region(dev(_to_c4(x)), None, w27, *geo, *bnd, in_c4=True, y_bound=bw[0])
        ybp = ops.conv3d_region(dev(_to_c4(x)), None, w27, *geo, *bnd, in_c4=True, per_lane=True)
        yc = ops.conv3d_region(spd, None, w27, *geo, *bnd, in_c4=True, absmax=wordsd)
        yd = ops.conv3d_region_split(spd, None, w27, *geo, wordsd, None, bw[1], *bnd)
        ydp = ops.conv3d_region_split(spd, None, w27, *geo, wordsd, None, bw[2], *bnd, per_lane=True)
        if cout == 16:
            ye = ops.conv_s2_split(dev(_to_c4(x)), wordsd, wd, cx.dims, org(out_reg), size(out_reg), cx.pad, *bnd)
            yf = ops.conv_s2_split(spd, wordsd, wd, cx.dims, org(out_reg), size(out_reg), cx.pad, *bnd)
        torch.cuda.synchronize()
    check_fp32(cf(ya, False), ref, reft, "ncdhw")
    e_b = check_fp32(cf(yb, False), ref, reft, "c4")
    e_c = check_fp32(cf(yc, False), refs, refts, "split volume")
    assert torch.equal(yb, ybp)
    assert bound_of(bw[0]) == yb.abs().max().item()
    check_split(cf(yd, False), refs, e_c, "region_split")
    assert torch.equal(yd, ydp)
    assert bound_of(bw[1]) == bound_of(bw[2]) == yd.abs().max().item()
    if cout == 16:
        check_split(cf(ye, False), ref, e_b, "conv_s2_split c4")
        check_split(cf(yf, False), refs, e_c, "conv_s2_split split volume")


def _s1_eval(cx, c, reg, halo):
    """conv_k_1 + BN + ReLU onto reg from its halo: channels-last and channels-first, fp32 and split."""
    from mvs_amd import ops
    x = zero_ext(cx.g, cx.b, c, cx.n, halo)
    wt = cx.randn(c, c, 3, 3, 3) * 0.1
    bn = cx.bn(c)
    f = lambda xx, ww: _bn_relu(F.conv3d(xx, ww, padding=1), *(t.to(xx.dtype) for t in bn))[sl(reg)]
    ref, reft = f(x.double(), wt.double()), f(x, wt)
    w27, bnd, xr = dev(conv_w27(wt)), dev(*bn), dev(cl(x[sl(halo)]))
    geo = (ops.CONV_S1, cx.dims, org(reg), size(reg), org(halo), size(halo), None)
    bw = ops.bound_words(5, DEV)
    set_bound(bw[0], xr)
    with torch.no_grad():
        y = ops.conv3d_region(xr, None, w27, *geo, *bnd, y_bound=bw[1])
        yn = ops.conv3d_region(xr, None, w27, *geo, *bnd, out_ncdhw=True)
        yp = ops.conv3d_region(xr, None, w27, *geo, *bnd, y_bound=bw[2], per_lane=True)
        s = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, bw[3], *bnd)
        sn = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, None, *bnd, out_ncdhw=True)
        sp = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, bw[4], *bnd, per_lane=True)
        torch.cuda.synchronize()
    e32 = check_fp32(cf(y, False), ref, reft, "cl")
    e32n = check_fp32(cf(yn, True), ref, reft, "ncdhw")
    assert torch.equal(y, yp)
    assert bound_of(bw[1]) == bound_of(bw[2]) == y.abs().max().item()
    check_split(cf(s, False), ref, e32, "cl")
    check_split(cf(sn, True), ref, e32n, "ncdhw")
    assert torch.equal(s, sp)
    assert bound_of(bw[3]) == bound_of(bw[4]) == s.abs().max().item()


def _t2_eval(cx, cin, cout, in_reg, out_reg, two):
    """deconv_3_0 (C3 -> C2) / deconv_2_0 (C2 -> B, the input a sum of two region tensors) + BN + ReLU:
    both layouts, fp32 and split; the split kernel also with the output addend (y_addend)."""
    from mvs_amd import ops
    r = cx.r
    x = zero_ext(cx.g, cx.b, cin, cx.n, in_reg)
    x2 = zero_ext(cx.g, cx.b, cin, cx.n, in_reg) if two else None
    add = torch.relu(cx.randn(cx.b, cout, *size(out_reg)))
    wt = cx.randn(cin, cout, 3, 3, 3) * 0.1
    bn = cx.bn(cout)
    f = lambda xx, ww: _bn_relu(F.conv_transpose3d(xx, ww, stride=2, padding=r.pad, output_padding=r.outpad),
                                *(t.to(xx.dtype) for t in bn))[sl(out_reg)]
    xin = x + x2 if two else x
    ref, reft = f(xin.double(), wt.double()), f(xin, wt)
    ref1, reft1 = f(x.double(), wt.double()), f(x, wt)    # one input: the y_addend form
    w27, bnd = dev(tconv_w27(wt)), dev(*bn)
    xr, x2r = dev(cl(x[sl(in_reg)])), dev(cl(x2[sl(in_reg)])) if two else None
    geo = (ops.CONV_T2, cx.dims, org(out_reg), size(out_reg), org(in_reg), size(in_reg), cx.pad)
    bw = ops.bound_words(6, DEV)
    set_bound(bw[0], xr)
    xb2 = set_bound(bw[1], x2r) if two else None
    addd, addn = dev(cl(add)), dev(add)
    with torch.no_grad():
        y = ops.conv3d_region(xr, x2r, w27, *geo, *bnd, y_bound=bw[2])
        yn = ops.conv3d_region(xr, x2r, w27, *geo, *bnd, out_ncdhw=True)
        yp = ops.conv3d_region(xr, x2r, w27, *geo, *bnd, per_lane=True)
        y1 = ops.conv3d_region(xr, None, w27, *geo, *bnd)
        s = ops.conv3d_region_split(xr, x2r, w27, *geo, bw[0], xb2, bw[3], *bnd)
        sn = ops.conv3d_region_split(xr, x2r, w27, *geo, bw[0], xb2, None, *bnd, out_ncdhw=True)
        sp = ops.conv3d_region_split(xr, x2r, w27, *geo, bw[0], xb2, bw[4], *bnd, per_lane=True)
        sa = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, bw[5], *bnd, y_addend=addd)
        san = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, None, *bnd, out_ncdhw=True, y_addend=addn)
        torch.cuda.synchronize()
    e32 = check_fp32(cf(y, False), ref, reft, "cl")
    e32n = check_fp32(cf(yn, True), ref, reft, "ncdhw")
    e321 = check_fp32(cf(y1, False), ref1, reft1, "one input")
    assert torch.equal(y, yp)
    assert bound_of(bw[2]) == y.abs().max().item()
    check_split(cf(s, False), ref, e32, "cl")
    check_split(cf(sn, True), ref, e32n, "ncdhw")
    assert torch.equal(s, sp)
    assert bound_of(bw[3]) == bound_of(bw[4]) == s.abs().max().item()
    check_split(cf(sa, False), ref1 + add.double(), e321, "y_addend cl")
    check_split(cf(san, True), ref1 + add.double(), e321, "y_addend ncdhw")
    assert bound_of(bw[5]) == sa.abs().max().item()


def _deconv(cx, bn_on):
    """deconv_1_0 from B into the full volume (deconv3d_k3s2).  Eval: + BN_0 + ReLU + y0, from the NCDHW
    region tensor and from the channels-last pair (x, x2).  Train: raw, the NCDHW pair (x, x2)."""
    from mvs_amd import ops
    r = cx.r
    reg = r.B
    x = zero_ext(cx.g, cx.b, 16, cx.n, reg, relu=False)
    x2 = zero_ext(cx.g, cx.b, 16, cx.n, reg, relu=False)
    wt = cx.randn(16, 8, 3, 3, 3) * 0.1
    bn = cx.bn(8)
    y0 = cx.randn(cx.b, 8, *cx.n)
    tc = lambda xx, ww: F.conv_transpose3d(xx, ww, stride=2, padding=r.pad, output_padding=r.outpad)
    if bn_on:
        f = lambda xx, ww: _bn_relu(tc(xx, ww), *(t.to(xx.dtype) for t in bn)) + y0.to(xx.dtype)
    else:
        f = tc
    xa, xb = dev(x[sl(reg)].contiguous()), dev(x2[sl(reg)].contiguous())
    wd, bnd, y0d = dev(wt), dev(*bn), dev(y0)
    with torch.no_grad():
        if bn_on:
            ya = ops.deconv3d_k3s2(xa, org(reg), wd, cx.dims, cx.pad, *bnd, y0d)
            yb = ops.deconv3d_k3s2(dev(cl(x[sl(reg)])), org(reg), wd, cx.dims, cx.pad, *bnd, y0d,
                                   x2=dev(cl(x2[sl(reg)])), channels_last=True)
        else:
            ya = ops.deconv3d_k3s2(xa, org(reg), wd, cx.dims, cx.pad, None, None, None, None)
            yb = ops.deconv3d_k3s2(xa, org(reg), wd, cx.dims, cx.pad, None, None, None, None, x2=xb)
        torch.cuda.synchronize()
    check_fp32(ya.cpu(), f(x.double(), wt.double()), f(x, wt), "one input")
    check_fp32(yb.cpu(), f((x + x2).double(), wt.double()), f(x + x2, wt), "two inputs")


def _s2_train(cx):
    """conv_1_0 / conv_2_0 / conv_3_0 raw onto R2 = grow(M, 2): conv3d_region from the NCDHW, channel-quad
    and split volumes; the three in one launch from the split volume with their batch sums and bound."""
    from mvs_amd import ops
    r = cx.r
    x, words, sp, xs = _s2_inputs(cx)
    wts = [cx.randn(c, 32, 3, 3, 3) * s for c, s in ((16, 0.1), (32, 0.03), (64, 0.2))]
    f = lambda xx, ww: F.conv3d(xx, ww, stride=2, padding=r.pad)[sl(r.R2)]
    w27s = [dev(conv_w27(w)) for w in wts]
    geo = (ops.CONV_S2, cx.dims, org(r.R2), size(r.R2), None, None, cx.pad)
    wordsd, spd = dev(words), dev(sp)
    bw = ops.bound_words(1, DEV)
    with torch.no_grad():
        ya = [ops.conv3d_region(dev(x), None, w, *geo) for w in w27s]
        yb = [ops.conv3d_region(dev(_to_c4(x)), None, w, *geo, in_c4=True) for w in w27s]
        yc = [ops.conv3d_region(spd, None, w, *geo, in_c4=True, absmax=wordsd) for w in w27s]
        multi = ops.conv_s2_split_multi_sums(spd, w27s, cx.dims, org(r.R2), size(r.R2), cx.pad, wordsd, y_bound=bw[0])
        torch.cuda.synchronize()
    for k, wt in enumerate(wts):
        ref, reft = f(x.double(), wt.double()), f(x, wt)
        refs, refts = f(xs.double(), wt.double()), f(xs, wt)
        check_fp32(cf(ya[k], False), ref, reft, "ncdhw %d" % k)
        check_fp32(cf(yb[k], False), ref, reft, "c4 %d" % k)
        e_c = check_fp32(cf(yc[k], False), refs, refts, "split volume %d" % k)
        y, s1, s2 = multi[k]
        check_split(cf(y, False), refs, e_c, "multi %d" % k)
        check_sums(s1, s2, cf(y, False), refs, "multi %d" % k)
    assert bound_of(bw[0]) == max(y.abs().max().item() for y, _, _ in multi)


def _crop(t, reg, want):
    return t[(slice(None), slice(None)) + tuple(slice(lo - rlo, hi - rlo + 1) for (rlo, _), (lo, hi) in zip(reg, want))]


def _in_bn(ps, cin):
    """ops.conv3d_region_split's in_bn rows for one or two folded input BNs (conv3d_region_split_sums)."""
    one, zero = torch.ones(cin), torch.zeros(cin)
    rows = list(ps[0]) + (list(ps[1]) if len(ps) > 1 else [one, zero, zero])
    return dev(torch.stack(rows).float().contiguous())


def _s1_train(cx, c):
    """conv_k_1 raw on R1 from R2 with the store box M.  fp32: the whole R1 output, cropped by
    regions._crop_*.  Split: the sums over R1 in the epilogue and only M stored; for 16 / 32 channels also
    with conv_k_0's BN + ReLU folded into the staging (x_bn)."""
    from mvs_amd import ops
    from mvs_amd.regions import _crop_cf, _crop_cl
    r = cx.r
    ncdhw = c == 16   # level 1 is channels-first (it only feeds deconv_1_0)
    raw = zero_ext(cx.g, cx.b, c, cx.n, r.R2, relu=False)
    p = cx.bn(c)
    x = torch.zeros_like(raw)
    x[sl(r.R2)] = _bn_relu(raw, *p)[sl(r.R2)]   # relu(BN(raw)) on R2; outside the volume stays the conv's zero padding
    wt = cx.randn(c, c, 3, 3, 3) * 0.1
    f = lambda xx, ww: F.conv3d(xx, ww, padding=1)[sl(r.R1)]
    ref, reft = f(x.double(), wt.double()), f(x, wt)
    w27 = dev(conv_w27(wt))
    xr, rawr = dev(cl(x[sl(r.R2)])), dev(cl(raw[sl(r.R2)]))
    geo = (ops.CONV_S1, cx.dims, org(r.R1), size(r.R1), org(r.R2), size(r.R2), None)
    box = dict(store_origin=org(r.M), store_size=size(r.M))
    bw = ops.bound_words(4, DEV)
    set_bound(bw[0], xr)
    set_bound(bw[1], rawr)
    fold = c in (16, 32)
    with torch.no_grad():
        y = ops.conv3d_region(xr, None, w27, *geo, out_ncdhw=ncdhw)
        yp = ops.conv3d_region(xr, None, w27, *geo, out_ncdhw=ncdhw, per_lane=True)
        ym = (_crop_cf if ncdhw else _crop_cl)(y, r.R1, r.M)
        s = ops.conv3d_region_split(xr, None, w27, *geo, bw[0], None, None, out_ncdhw=ncdhw)
        sb, s1, s2 = ops.conv3d_region_split_sums(xr, None, w27, *geo, bw[0], out_ncdhw=ncdhw,
                                                  y_bound=None if ncdhw else bw[2], **box)
        if fold:
            fb, f1, f2 = ops.conv3d_region_split_sums(rawr, None, w27, *geo, bw[1], out_ncdhw=ncdhw,
                                                      y_bound=None if ncdhw else bw[3], x_bn=dev(*p), **box)
        torch.cuda.synchronize()
    e32 = check_fp32(cf(y, ncdhw), ref, reft, "R1")
    assert torch.equal(y, yp)
    refm = _crop(ref, r.R1, r.M)
    assert torch.equal(cf(ym, ncdhw), _crop(cf(y, ncdhw), r.R1, r.M)) and ym.is_contiguous()
    errs(cf(ym, ncdhw), refm)
    check_split(cf(s, ncdhw), ref, e32, "R1")
    assert torch.equal(cf(sb, ncdhw), _crop(cf(s, ncdhw), r.R1, r.M))   # the stored box: that output's crop
    check_sums(s1, s2, cf(s, ncdhw), ref, "sums")
    if not ncdhw:
        assert bound_of(bw[2]) == sb.abs().max().item()
    if fold:
        scale = ref.abs().max().item()
        assert (fb - sb).abs().max().item() <= 2e-6 * scale
        assert errs(cf(fb, ncdhw), refm)[0] <= 1e-5 * scale
        torch.testing.assert_close(f1, s1, rtol=1e-5, atol=1e-5 * scale)
        torch.testing.assert_close(f2, s2, rtol=1e-5, atol=1e-5 * scale * scale)
        if not ncdhw:
            assert bound_of(bw[3]) == fb.abs().max().item()


def _t2_train(cx, cin, cout, two):
    """deconv_3_0 / deconv_2_0 raw from M onto the full volume (out_origin 0, out_size n), M stored.  fp32:
    the full output, cropped.  Split: sums over the full volume, store box M, bound words; and with the
    BN + ReLU of the input(s) folded into the staging (x_bn / x2_bn)."""
    from mvs_amd import ops
    from mvs_amd.regions import _crop_cf, _crop_cl
    r = cx.r
    ncdhw = two   # deconv_2_0's output is channels-first
    raws = [zero_ext(cx.g, cx.b, cin, cx.n, r.M, relu=False) for _ in range(2 if two else 1)]
    ps = [cx.bn(cin) for _ in raws]
    xs = []
    for raw, p in zip(raws, ps):
        x = torch.zeros_like(raw)
        x[sl(r.M)] = _bn_relu(raw, *p)[sl(r.M)]
        xs.append(x)
    wt = cx.randn(cin, cout, 3, 3, 3) * 0.1
    f = lambda xx, ww: F.conv_transpose3d(xx, ww, stride=2, padding=r.pad, output_padding=r.outpad)
    xin = xs[0] + xs[1] if two else xs[0]
    ref, reft = f(xin.double(), wt.double()), f(xin, wt)
    assert tuple(ref.shape[2:]) == cx.n
    w27 = dev(tconv_w27(wt))
    xr = [dev(cl(x[sl(r.M)])) for x in xs]
    rr = [dev(cl(x[sl(r.M)])) for x in raws]
    x2r, r2r = (xr[1], rr[1]) if two else (None, None)
    geo = (ops.CONV_T2, cx.dims, [0, 0, 0], cx.dims, org(r.M), size(r.M), cx.pad)
    box = dict(store_origin=org(r.M), store_size=size(r.M))
    bw = ops.bound_words(6, DEV)
    set_bound(bw[0], xr[0])
    set_bound(bw[2], rr[0])
    if two:
        set_bound(bw[1], xr[1])
        set_bound(bw[3], rr[1])
    b1, b3 = (bw[1], bw[3]) if two else (None, None)
    with torch.no_grad():
        y = ops.conv3d_region(xr[0], x2r, w27, *geo, out_ncdhw=ncdhw)
        yp = ops.conv3d_region(xr[0], x2r, w27, *geo, out_ncdhw=ncdhw, per_lane=True)
        ym = (_crop_cf if ncdhw else _crop_cl)(y, r.full, r.M)
        s = ops.conv3d_region_split(xr[0], x2r, w27, *geo, bw[0], b1, None, out_ncdhw=ncdhw)
        sb, s1, s2 = ops.conv3d_region_split_sums(xr[0], x2r, w27, *geo, bw[0], x2_bound=b1, out_ncdhw=ncdhw,
                                                  y_bound=bw[4], **box)
        fb, f1, f2 = ops.conv3d_region_split_sums(rr[0], r2r, w27, *geo, bw[2], x2_bound=b3, out_ncdhw=ncdhw,
                                                  y_bound=bw[5], x_bn=dev(*ps[0]),
                                                  x2_bn=dev(*ps[1]) if two else None, **box)
        torch.cuda.synchronize()
    e32 = check_fp32(cf(y, ncdhw), ref, reft, "full")
    assert torch.equal(y, yp)
    refm = _crop(ref, r.full, r.M)
    assert torch.equal(cf(ym, ncdhw), _crop(cf(y, ncdhw), r.full, r.M)) and ym.is_contiguous()
    check_split(cf(s, ncdhw), ref, e32, "full")
    assert torch.equal(cf(sb, ncdhw), _crop(cf(s, ncdhw), r.full, r.M))
    check_sums(s1, s2, cf(s, ncdhw), ref, "sums")
    assert bound_of(bw[4]) == sb.abs().max().item()
    scale = ref.abs().max().item()
    assert (fb - sb).abs().max().item() <= 2e-6 * scale
    assert errs(cf(fb, ncdhw), refm)[0] <= 1e-5 * scale
    torch.testing.assert_close(f1, s1, rtol=1e-5, atol=1e-5 * scale)
    torch.testing.assert_close(f2, s2, rtol=1e-5, atol=1e-5 * scale * scale)
    assert bound_of(bw[5]) == fb.abs().max().item()


LAYERS = {
    # the eval chain (_forward_live_hip)
    "eval_s2_16": lambda cx: _s2_eval(cx, 16, cx.r.hB),
    "eval_s2_32": lambda cx: _s2_eval(cx, 32, cx.r.hC2),
    "eval_s2_64": lambda cx: _s2_eval(cx, 64, cx.r.hC3),
    "eval_s1_16": lambda cx: _s1_eval(cx, 16, cx.r.B, cx.r.hB),
    "eval_s1_32": lambda cx: _s1_eval(cx, 32, cx.r.C2, cx.r.hC2),
    "eval_s1_64": lambda cx: _s1_eval(cx, 64, cx.r.C3, cx.r.hC3),
    "eval_t2_64_32": lambda cx: _t2_eval(cx, 64, 32, cx.r.C3, cx.r.C2, False),
    "eval_t2_32_16": lambda cx: _t2_eval(cx, 32, 16, cx.r.C2, cx.r.B, True),
    "eval_deconv": lambda cx: _deconv(cx, True),
    # the train chain (_forward_live_train_hip)
    "train_s2": _s2_train,
    "train_s1_16": lambda cx: _s1_train(cx, 16),
    "train_s1_32": lambda cx: _s1_train(cx, 32),
    "train_s1_64": lambda cx: _s1_train(cx, 64),
    "train_t2_64_32": lambda cx: _t2_train(cx, 64, 32, False),
    "train_t2_32_16": lambda cx: _t2_train(cx, 32, 16, True),
    "train_deconv": lambda cx: _deconv(cx, False),
}


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("n", GEOMETRIES, ids=gid)
def test_region_layer(n, layer):
    LAYERS[layer](Cx(n, list(LAYERS).index(layer)))


# ---- part 2: the whole chain --------------------------------------------------------------------------
def _model(n):
    from test_regulariser_live import _reg
    return _reg(*n, seed=sum(n))


@functools.lru_cache(maxsize=None)
def _chain_reference(n, mode, batch):
    """(cv, float64 forward_full probabilities, the BN state afterwards) on the CPU, computed once."""
    m = _model(n)
    m = m.train() if mode == "train" else m.eval()
    cv = torch.rand(batch, 32, *n, generator=torch.Generator().manual_seed(100 * n[0] + n[2] + batch))
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        ref = m64.forward_full(cv.double())
    return cv, ref, {k: v.clone() for k, v in m64.state_dict().items() if "BN_" in k}


def _rel(y, ref):
    return ((y.double().cpu() - ref).abs() / ref.abs()).max().item()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("arithmetic", ["fp32", "split_f16"])
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("n", GEOMETRIES, ids=gid)
def test_live_chain(n, mode, arithmetic, batch, monkeypatch):
    """CostVolumeReg on the HIP live path against float64 forward_full, per input form.  (1, 2, 3) has
    D = 1: the softmax over depth is 1 everywhere, so its probability comparison is vacuous -- it is kept
    for the shape, finiteness and the running statistics, not as chain coverage (part 1 covers its kernels)."""
    from conftest import record_parity
    from mvs_amd import ops
    from mvs_amd.regulariser import CostVolumeReg
    cv, ref, ref_state = _chain_reference(tuple(n), mode, batch)
    train = mode == "train"
    split = arithmetic == "split_f16"
    words = volume_bound_words(cv)
    c4 = _to_c4(cv)
    forms = {"ncdhw": lambda: dev(cv), "c4": lambda: ops.BoundCostVolume(dev(c4), dev(words))}
    if split:
        forms["split"] = lambda: ops.BoundCostVolume(dev(split_volume(c4, words)), dev(words))
    ran = []
    for name in ("_forward_live_hip", "_forward_live_train_hip"):
        fn = getattr(CostVolumeReg, name)

        def counted(self, *a, _fn=fn, _name=name, **k):
            ran.append(_name)
            return _fn(self, *a, **k)
        monkeypatch.setattr(CostVolumeReg, name, counted)
    monkeypatch.setattr(CostVolumeReg, "forward_full", lambda self, cv: pytest.fail("fell back to forward_full"))
    want = "_forward_live_train_hip" if train else "_forward_live_hip"
    base = _model(tuple(n))
    base = (base.train() if train else base.eval()).to(DEV)

    def run(form, split_f16):
        m = copy.deepcopy(base)   # (train mode updates the running statistics: one module per forward)
        m.split_f16 = split_f16
        x = forms[form]()
        with torch.no_grad():
            assert m.live_train_ok(n) if train else m.live_ok(n)
            if form == "split":
                assert m._split_head_ok(x.data, n) == (tuple(n) == (20, 32, 40))
            del ran[:]
            y = m(x)
            torch.cuda.synchronize()
        assert ran == [want], ran
        assert y.shape == ref.shape and torch.isfinite(y).all()
        return y.cpu(), {k: v.cpu() for k, v in m.state_dict().items() if "BN_" in k}

    def stat_err(state):
        return {k: (state[k].double() - v).abs().max().item() for k, v in ref_state.items() if "num_batches" not in k}

    worst = 0.0
    for form in forms:
        y32, st32 = run(form, False) if (not split or train) else (None, None)
        if not split:
            y, st = y32, st32
        else:
            y, st = run(form, True)
        rel = _rel(y, ref)
        worst = max(worst, rel)
        print("%s %s %s B=%d %s: max rel err %.3g" % (gid(n), mode, arithmetic, batch, form, rel))
        if split:
            torch.testing.assert_close(y.double(), ref, rtol=2e-3, atol=1e-7)
        else:
            torch.testing.assert_close(y.double(), ref, rtol=1e-4, atol=1e-6 if train else 1e-7)
        if train:
            for k, v in ref_state.items():
                if "num_batches" in k:
                    assert st[k].item() == v.item(), k
                elif not split:
                    torch.testing.assert_close(st[k].double(), v, rtol=1e-5, atol=1e-6, msg=lambda s, k=k: k + " " + s)
                else:
                    e, e32 = stat_err(st)[k], stat_err(st32)[k]
                    assert e <= 2 * e32 + 1e-6 + 1e-5 * v.abs().max().item(), (k, e, e32)
    record_parity("region_geometry_chain_%s_%s_%s_b%d" % (gid(n), mode, arithmetic, batch), max_rel_err=worst,
                  vacuous=n[0] == 1)
