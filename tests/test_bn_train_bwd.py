"""GPU: the train-mode BatchNorm + ReLU site under autograd on the HIP kernels (mvs_amd/bn_train.py bn_relu_train:
ops.channel_stats and ops.bn_relu_ forward, csrc/bn_train_bwd.hip's reduce and apply kernels backward).

Reference: float64 autograd of the torch expressions the site replaces (bn_sums._sums, _bn_train, _apply_bn, the
ReLU, regions._crop_pad), with the ReLU mask taken from the HIP forward's output -- a fp32 pre-activation within
rounding of 0 is not a gradient error; a separate assertion pins that mask to the float64 one wherever
|pre64| > 1e-5 ((|z| + |mean|) |scale| + |shift|).

Criterion for out, gz, g_weight, g_bias, g_c1, g_c2 (test_gpu_train.py's rule): the max error against float64, relative
to the float64 result's max magnitude, is at most 2 x that of the fp32 torch path on the same device with the same
inputs and the same mask, + 2^-23: one ulp of an fp32 result at the max magnitude (a float64-accumulated sum rounded
once to fp32 is not asked to beat an fp32 sum that happens to land closer).  Measured errors: DESIGN.md 3.6.

The constants below MIRROR csrc/bn_train_bwd.hip: 256 threads per workgroup; channels-last items are float4s of all
of gy (reduce) or z (apply), at most 2048 workgroups; NCDHW items are float4s of a plane when there is no box and the
plane is a multiple of 4, single voxels otherwise, about 2048 / (B C) workgroups per plane.  The multi-pass case
asserts its pass count through the slots query, so a change of the grids fails there.

Mutation runs (scratch builds, not committed) are recorded in DESIGN.md 3.6."""
import copy
import ctypes
import functools

import pytest
import torch

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
BLOCK = 256
ULP = 2.0 ** -23


def _as_cl(t):
    """A logical NCDHW tensor over channels-last memory."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def _in_layout(t, layout):
    return _as_cl(t) if layout == "channels_last" else t.contiguous()


def _boxes(dims):
    D, H, W = dims
    return {"none": None, "whole": ((0, D - 1), (0, H - 1), (0, W - 1)), "low_corner": ((0, 0), (0, 0), (0, 0)),
            "high_corner": ((D - 2, D - 1), (H - 3, H - 1), (W - 4, W - 1)), "interior": ((1, D - 2), (2, H - 2), (1, W - 3))}


def _box_shape(dims, box):
    return tuple(dims) if box is None else tuple(hi - lo + 1 for lo, hi in box)


def _bn(C, seed, eps=1e-5):
    """BatchNorm3d in train mode: weights of mixed sign, channel 2's weight 0."""
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm3d(C, eps=eps, momentum=0.1)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=g))
        bn.weight[2] = 0.0
        bn.weight[0], bn.weight[3] = 0.8, -1.1
        bn.bias.copy_(0.5 * torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn.train()


def _inputs(C, B, dims, seed):
    """z with channel 1 constant (its variance is 0: the clamp), gy per box, the border term."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, *dims, generator=g) * 1.5 + 0.3 * torch.randn(1, C, 1, 1, 1, generator=g)
    z[:, 1] = 0.1
    extra = (torch.randn(C, generator=g).double() * 40.0, torch.rand(C, generator=g).double() * 900.0 + 100.0)
    return z, extra, g


def _torch_path(z, bn, extra, count, box, gy, mask=None, tail=None):
    """The torch expressions of CostVolumeReg.forward_live_train for one site, in z's dtype, and their autograd
    gradients for the loss sum(out * gy) [+ tail(p)]; ``mask``: the ReLU as a product with this 0/1 mask."""
    from mvs_amd.bn_sums import _apply_bn, _bn_train, _sums
    from mvs_amd.regions import _crop_pad
    z = z.detach().clone().requires_grad_(True)
    c = [None, None] if extra is None else [t.detach().clone().requires_grad_(True) for t in extra]
    s1, s2 = _sums(z)
    if extra is not None:
        s1, s2 = s1 + c[0], s2 + c[1]
    p = _bn_train(bn, s1, s2, count)
    n = tuple(z.shape[2:])
    full = tuple((0, d - 1) for d in n)
    pre = _apply_bn(z if box is None else _crop_pad(z, full, box, n), *p)
    out = torch.relu(pre) if mask is None else pre * mask.to(pre.dtype)
    loss = (out * gy.to(out.dtype)).sum()
    if tail is not None:
        loss = loss + tail(p)
    loss.backward()
    res = {"out": out.detach(), "gz": z.grad, "g_weight": bn.weight.grad, "g_bias": bn.bias.grad}
    if extra is not None:
        res["g_c1"], res["g_c2"] = c[0].grad, c[1].grad
    return res, pre.detach(), [t.detach() for t in p]


def _hip_path(z, bn, extra, count, box, gy, tail=None):
    from mvs_amd.bn_train import bn_relu_train
    z = z.detach().requires_grad_(True)
    c = None if extra is None else tuple(t.detach().clone().requires_grad_(True) for t in extra)
    out, p = bn_relu_train(z, box, bn, c, count)
    loss = (out * gy).sum()
    if tail is not None:
        loss = loss + tail(p)
    loss.backward()
    res = {"out": out.detach(), "gz": z.grad, "g_weight": bn.weight.grad, "g_bias": bn.bias.grad}
    if extra is not None:
        res["g_c1"], res["g_c2"] = c[0].grad, c[1].grad
    return res, [t.detach() for t in p]


def _compare(what, z, bn, extra, count, box, gy, layout, tail=None, measured=None):
    """HIP against float64 by the criterion; returns the HIP results."""
    zg = _in_layout(z.to(DEV), layout)
    ex = None if extra is None else tuple(t.to(DEV) for t in extra)
    gyg = gy.to(DEV)
    bn_h, bn_t, bn_d = copy.deepcopy(bn).to(DEV), copy.deepcopy(bn).to(DEV), copy.deepcopy(bn).double().to(DEV)
    hip, p_hip = _hip_path(zg, bn_h, ex, count, box, gyg, tail)
    mask = hip["out"] > 0
    ref, pre64, p64 = _torch_path(zg.double(), bn_d, ex, count, box, gyg.double(), mask, tail)
    t32, _, _ = _torch_path(zg, bn_t, ex, count, box, gyg, mask, tail)
    # the mask is the float64 one away from 0
    scale, shift, mean = (t.view(1, -1, 1, 1, 1) for t in p64)
    zb = zg.double() if box is None else zg.double()[(slice(None), slice(None)) + tuple(slice(lo, hi + 1) for lo, hi in box)]
    clear = pre64.abs() > 1e-5 * ((zb.abs() + mean.abs()) * scale.abs() + shift.abs())
    assert torch.equal(mask[clear], (pre64 > 0)[clear]), what
    assert zg.grad is None and hip["gz"].shape == zg.shape and hip["gz"].stride() == zg.stride(), what
    for key in ref:
        top = ref[key].abs().max().item()
        if top == 0.0:
            assert hip[key].abs().max().item() == 0.0, (what, key)
            continue
        e_h = (hip[key].double() - ref[key]).abs().max().item() / top
        e_t = (t32[key].double() - ref[key]).abs().max().item() / top
        if measured is not None:
            measured[key] = max(measured.get(key, (0.0, 0.0)), (e_h, e_t))
        print("%s %s: hip %.3g torch-fp32 %.3g (max |ref| %.3g)" % (what, key, e_h, e_t, top))
        assert e_h <= 2.0 * e_t + ULP, (what, key, e_h, e_t)
    # the running statistics move as _bn_train moves them
    for name in ("running_mean", "running_var"):
        torch.testing.assert_close(getattr(bn_h, name).double(), getattr(bn_d, name), rtol=1e-5, atol=1e-6)
    assert int(bn_h.num_batches_tracked) == int(bn.num_batches_tracked) + 1
    return hip


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ncdhw", "channels_last"])
@pytest.mark.parametrize("dims", [(5, 7, 9), (8, 12, 16)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [8, 16, 32, 64])
def test_site_matches_float64(C, B, dims, layout):
    """Every box (none, whole, one voxel at the low corner, touching the high corner, interior) with and without the
    border term; with it, the count exceeds z's own.  Channel 1 of z is constant (variance 0, the clamp), channel
    2's weight is 0, the weights have both signs."""
    z, extra, g = _inputs(C, B, dims, 100 * C + 10 * B + dims[0])
    bn = _bn(C, C + B)
    own = B * dims[0] * dims[1] * dims[2]
    measured = {}
    for name, box in _boxes(dims).items():
        gy = torch.randn((B, C) + _box_shape(dims, box), generator=g)
        for ex, count in ((None, own), (extra, own + 977)):
            _compare("C%d B%d %s %s %s%s" % (C, B, dims, layout, name, "" if ex is None else " +extra"), z, bn, ex, count,
                     box, gy, layout, measured=measured)
    print("worst (hip, torch-fp32) per result:", {k: ("%.3g" % a, "%.3g" % b) for k, (a, b) in measured.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ncdhw", "channels_last"])
def test_per_channel_outputs_carry_gradient(layout):
    """bn_sums._bn_constant of the node's (scale, shift, mean) -- the next layer's border term -- in the loss: its
    gradient reaches z, the BN's weight and bias and the border term through the same closed form."""
    from mvs_amd.bn_sums import _bn_constant
    C, B, dims = 16, 2, (5, 7, 9)
    z, extra, g = _inputs(C, B, dims, 5)
    v = torch.randn(C, generator=g) * 50.0
    tail = lambda p: (_bn_constant(p) * v.to(device=p[0].device, dtype=p[0].dtype)).sum()
    gy = torch.randn((B, C) + _box_shape(dims, _boxes(dims)["interior"]), generator=g)
    _compare("tail " + layout, z, _bn(C, 3), extra, B * 315 + 50, _boxes(dims)["interior"], gy, layout, tail)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ncdhw", "channels_last"])
def test_exact_cases(layout):
    """gy a single 1 at one box voxel.  weight = 0: scale and every g_s* are 0, gz is exactly 0 everywhere (the
    mask is on: bias > 0).  weight = 1 with eps = 2^40 and count = 2^80: scale = 2^-20 exactly, g_s1 and g_s2 are
    below 2^-99, so gz at that voxel is scale to the bit and nothing else reaches 2^-90."""
    from mvs_amd.bn_train import bn_relu_train
    C, B, dims = 8, 2, (5, 7, 9)
    box = _boxes(dims)["interior"]
    z = _in_layout((torch.randn(B, C, *dims, generator=torch.Generator().manual_seed(1))).to(DEV), layout)
    at = (1, 5, 2, 3, 4)   # (b, c, box voxel)
    vox = (1, 5, 2 + box[0][0], 3 + box[1][0], 4 + box[2][0])
    for weight, eps, count in ((0.0, 1e-5, B * 315), (1.0, 2.0 ** 40, 2.0 ** 80)):
        bn = torch.nn.BatchNorm3d(C, eps=eps).to(DEV).train()
        with torch.no_grad():
            bn.weight.fill_(weight)
            bn.bias.fill_(3.0)
        zz = z.detach().requires_grad_(True)
        out, (scale, _, _) = bn_relu_train(zz, box, bn, None, count)
        gy = torch.zeros_like(out)
        gy[at] = 1.0
        out.backward(gy)
        assert out[at] > 0
        if weight == 0.0:
            assert int(torch.count_nonzero(zz.grad)) == 0
        else:
            assert scale[5].item() == 2.0 ** -20
            assert zz.grad[vox].item() == scale[5].item()
            rest = zz.grad.clone()
            rest[vox] = 0.0
            assert rest.abs().max().item() < 2.0 ** -90


def _kernel_inputs(C, B, dims, box, layout, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = torch.randn((B, C) + tuple(dims), device=DEV, generator=g)
    gy = torch.randn((B, C) + _box_shape(dims, box), device=DEV, generator=g)
    vec = lambda s: torch.randn(C, device=DEV, generator=g) * s
    cl = layout == "channels_last"
    mem = (lambda t: t.permute(0, 2, 3, 4, 1).contiguous()) if cl else (lambda t: t)
    return mem(z), mem(gy), cl, (vec(1.0), vec(0.5), vec(0.3)), (vec(0.1), vec(0.05))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ncdhw", "channels_last"])
def test_kernels_reproducible_whatever_the_workspace_held(layout):
    from mvs_amd import ops
    C, B, dims = 16, 3, (9, 14, 21)
    box = _boxes(dims)["interior"]
    zm, gym, cl, p, gs = _kernel_inputs(C, B, dims, box, layout, 11)
    slots = ops.bn_relu_bwd_slots(zm, cl, box)
    assert slots > 1
    first = ops.bn_relu_bwd_reduce(zm, gym, cl, box, *p)
    gz = ops.bn_relu_bwd_apply(zm, gym, cl, box, *p, *gs)
    for value in (float("nan"), 0.0):
        ws = torch.full((slots, 2, C), value, device=DEV, dtype=torch.float64)
        again = ops.bn_relu_bwd_reduce(zm, gym, cl, box, *p, workspace=ws)
        assert bool(torch.isfinite(ws).all())
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
        assert torch.equal(gz, ops.bn_relu_bwd_apply(zm, gym, cl, box, *p, *gs))


def _passes(C, B, dims, box, cl):
    """[(passes of the longest-running workgroup, items left for the last pass)] of the reduce (over the box, its
    grid the slots query's) and of the apply (over all of z, its grid the slots query's for the whole volume)."""
    from mvs_amd import ops
    shape = torch.empty((B,) + tuple(dims) + (C,) if cl else (B, C) + tuple(dims), device="meta")
    vol = lambda s: s[0] * s[1] * s[2]
    res = []
    for vox, b in ((vol(_box_shape(dims, box)), box), (vol(dims), None)):
        slots = ops.bn_relu_bwd_slots(shape, cl, b)
        if cl:
            items, per = B * vox * C // 4, slots
        else:   # float4s of a plane when there is no box and it is a multiple of 4, single voxels otherwise
            items, per = (vox // 4 if box is None and vox % 4 == 0 else vox), slots // B
        res.append((-(-items // (per * BLOCK)), items % (per * BLOCK)))
    return res


# every workgroup at least three passes, the last one ragged: (37, 150, 143) channels-last (1,587,300 float4s over
# 2048 x 256 threads), (37, 150, 144) NCDHW (199,800 float4s of a plane over 256 x 256); with the box, (40, 150, 144)
MULTI = {"channels_last": (37, 150, 143), "ncdhw": (37, 150, 144)}
MULTI_BOX = ((40, 150, 144), ((1, 39), (0, 149), (0, 143)))


@pytest.mark.gpu
@pytest.mark.parametrize("boxed", [False, True])
@pytest.mark.parametrize("layout", ["ncdhw", "channels_last"])
def test_three_passes_match_float64(layout, boxed):
    C, B = 8, 1
    dims, box = MULTI_BOX if boxed else (MULTI[layout], None)
    for n, rest in _passes(C, B, dims, box, layout == "channels_last"):
        assert n >= 3 and rest != 0, (layout, boxed, n, rest)
    z, extra, g = _inputs(C, B, dims, 21)
    gy = torch.randn((B, C) + _box_shape(dims, box), generator=g)
    _compare("multi-pass %s boxed=%s" % (layout, boxed), z, _bn(C, 9), extra, z.numel() // C + 1000, box, gy, layout)


GB = 1 << 30
BIG = (2, 4, (512, 512, 513))   # 1,075,838,976 floats = 4,303,355,904 B > 2^32


@pytest.mark.gpu
def test_past_4gb():
    """z, gy and gz NCDHW of 4.30 GB each, box None: S_g and S_gz against float64 sums taken plane by plane under the
    HIP forward's mask, gz plane by plane against the closed form evaluated in float64 from the same fp32 inputs,
    within 2^-22 of the terms' magnitudes (three fp32 roundings).  Peak device memory about 23 GB."""
    from mvs_amd import ops
    B, C, dims = BIG
    plane = dims[0] * dims[1] * dims[2]
    assert B * C * plane * 4 > 1 << 32 and plane % 4 == 0
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 28 * GB:
        pytest.skip("%.1f GB free on the device; the test peaks at about 23 GB" % (free / GB))
    assert all(n >= 3 for n, _ in _passes(C, B, dims, None, False))
    z = gy = out = gz = None
    try:
        g = torch.Generator(device=DEV).manual_seed(3)
        z = torch.randn((B, C) + dims, device=DEV, generator=g)
        gy = torch.randn((B, C) + dims, device=DEV, generator=g)
        sc = torch.tensor([0.7, -1.3, 0.0, 2.0], device=DEV)
        sh = torch.tensor([0.2, 0.1, 1.0, -0.5], device=DEV)
        mu = torch.tensor([0.1, -0.2, 0.3, 0.0], device=DEV)
        g1 = torch.tensor([0.01, -0.02, 0.03, 0.0], device=DEV)
        g2 = torch.tensor([0.005, 0.0, -0.01, 0.02], device=DEV)
        out = ops.bn_relu_(z, False, sc, sh, mu, out=torch.empty_like(z))
        s_g, s_gz = ops.bn_relu_bwd_reduce(z, gy, False, None, sc, sh, mu)
        gz = ops.bn_relu_bwd_apply(z, gy, False, None, sc, sh, mu, g1, g2)
        r_g = torch.zeros(C, dtype=torch.float64, device=DEV)
        r_gz = torch.zeros(C, dtype=torch.float64, device=DEV)
        for b in range(B):
            for c in range(C):
                ga = torch.where(out[b, c] > 0, gy[b, c], torch.zeros((), device=DEV)).double()
                z64 = z[b, c].double()
                r_g[c] += ga.sum()
                r_gz[c] += (ga * z64).sum()
                t = (ga * sc[c].double()).abs() + g1[c].double().abs() + (2.0 * z64 * g2[c].double()).abs()
                want = ga * sc[c].double() + g1[c].double() + 2.0 * z64 * g2[c].double()
                bad = (gz[b, c].double() - want).abs() > 2.0 ** -22 * t
                assert not bool(bad.any()), (b, c, int(bad.sum()))
                del ga, z64, t, want, bad
        torch.testing.assert_close(s_g, r_g, rtol=1e-11, atol=1e-6)
        torch.testing.assert_close(s_gz, r_gz, rtol=1e-11, atol=1e-6)
    finally:
        del z, gy, out, gz
        torch.cuda.empty_cache()


def _size(*v):
    return (ctypes.c_int * 3)(*v)


def test_backward_arguments_rejected_before_any_launch():
    """No GPU needed: unsupported arguments come back as the project's negative codes before anything is launched."""
    from mvs_amd import _lib
    lib = _lib.load()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    dims, org, size = _size(5, 7, 9), _size(1, 2, 3), _size(4, 5, 6)
    CL = _lib.MVS_LAYOUT_CHANNELS_LAST

    def reduce(z=fake, gy=fake, layout=0, batch=2, channels=8, dims=dims, org=org, size=size, sc=fake, sh=fake, mu=fake,
               stats=fake):
        return lib.mvs_bn_relu_bwd_reduce(z, gy, layout, batch, channels, dims, org, size, sc, sh, mu, stats, null)

    def apply(z=fake, gy=fake, layout=0, batch=2, channels=8, dims=dims, org=org, size=size, sc=fake, sh=fake, mu=fake,
              g1=fake, g2=fake, gz=fake):
        return lib.mvs_bn_relu_bwd_apply(z, gy, layout, batch, channels, dims, org, size, sc, sh, mu, g1, g2, gz, null)

    def slots(layout=0, batch=2, channels=8, dims=dims, org=org, size=size):
        return lib.mvs_bn_relu_bwd_slots(layout, batch, channels, dims, org, size)
    for call, pointers, aligned in ((reduce, ("z", "gy", "sc", "sh", "mu", "stats"), ("z", "gy")),
                                    (apply, ("z", "gy", "sc", "sh", "mu", "g1", "g2", "gz"), ("z", "gy", "gz"))):
        for name in pointers:
            assert call(**{name: null}) == -1, name
        for name in aligned:
            assert call(**{name: odd}) == -1, name
    assert slots() > 0 and slots(layout=CL) > 0 and slots(org=None, size=None) > 0
    for call, bad in ((reduce, -1), (apply, -1), (slots, 0)):
        for c in (6, 9, 1, 12, 260):                                   # channels-last: C = 4 x a power of two <= 256
            assert call(layout=CL, channels=c) == bad, c
        assert call(layout=2) == bad and call(batch=0) == bad and call(channels=0) == bad
        assert call(dims=None) == bad and call(dims=_size(5, 0, 9)) == bad
        assert call(org=None) == bad and call(size=None) == bad       # the box: both or neither
        assert call(org=_size(-1, 2, 3)) == bad                        # a box outside the extents
        assert call(org=_size(2, 2, 3)) == bad and call(size=_size(4, 5, 7)) == bad
        assert call(size=_size(4, 0, 6)) == bad and call(size=_size(6, 5, 6)) == bad
    assert reduce(batch=8192, channels=8) == -3 and apply(batch=8192, channels=8) == -3   # NCDHW planes past 65535
    assert slots(batch=8192, channels=8) == 0


def test_bn_relu_train_refuses_cpu_tensors_and_bad_boxes():
    """No fallback: a CPU tensor is an error, and a box outside the extents never reaches the library."""
    from mvs_amd import _lib
    from mvs_amd.bn_train import bn_relu_train
    bn = _bn(8, 1)
    z = torch.zeros(1, 8, 3, 4, 5)
    with pytest.raises(_lib.MVSLibraryError):
        bn_relu_train(z, None, bn, None, 60)
    for box in (((0, 3), (0, 3), (0, 4)), ((-1, 2), (0, 3), (0, 4)), ((2, 1), (0, 3), (0, 4))):
        with pytest.raises(ValueError):
            bn_relu_train(z, box, bn, None, 60)
    assert int(bn.num_batches_tracked) == 0   # nothing was updated on the way to the error
