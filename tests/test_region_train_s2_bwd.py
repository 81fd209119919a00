"""GPU: the stacked stride-2 region convolution's HIP backward (MVS_TRAIN_S2_BWD=hip; mvs_amd/region_train.py
_S2Box: the weight gradient on csrc/conv3d_s2_wgrad.hip from the NCDHW volume in place, the input gradient on
the region kernel's transposed mode with four partial sums per output) against float64 torch autograd, both
gradients' placement on exact impulses, the weight gradient's bit-reproducibility whatever the workspace held,
the autograd routing with either forward, the default path unchanged, and the regulariser's whole chain.
(At most two passes of the weight gradient's tile loop; the multi-pass cases: test_region_train_multipass.py.)"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

# (B, dims, pad_lo, out_size): one output voxel (K = 1); odd extents, leading outputs that read only padding,
# trailing outputs past the volume's end, 17+ outputs along x; several samples with both pad_lo parities;
# deeper than wide
GEOMETRIES = [(1, (3, 3, 3), (0, 0, 0), (1, 1, 1)),
              (2, (5, 6, 35), (1, 2, 5), (4, 5, 21)),
              (3, (8, 7, 40), (0, 1, 0), (4, 4, 20)),
              (1, (11, 4, 9), (2, 0, 3), (7, 2, 6))]
IMPULSE_GEO = (2, (9, 10, 41), (1, 0, 1), (4, 5, 20))


def _conv64(x, w, pad_lo, out):
    """F.conv3d, stride 2, of x zero-padded by pad_lo on the low side and enough on the high side: output o
    reads inputs 2 o - pad_lo + t; the first `out` outputs per dim."""
    flat = []
    for n, p, o in reversed(list(zip(x.shape[2:], pad_lo, out))):   # F.pad order: W, H, D
        flat += [p, max(2 * o + 1 - (p + n), 0)]
    y = F.conv3d(F.pad(x, flat), w, stride=2)
    return y[:, :, :out[0], :out[1], :out[2]]


@functools.lru_cache(maxsize=None)
def _reference(geo, seed):
    """Inputs and the float64 CPU results (y, gx, gw) with the same sums over absolute values, computed once."""
    b, dims, pad_lo, out = geo
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 32, *dims, generator=g)
    w = torch.randn(112, 32, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, 112, *out, generator=g)
    res = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        x64, w64 = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y64 = _conv64(x64, w64, pad_lo, out)
        (y64 * f(gy)).sum().backward()
        res.append((y64.detach(), x64.grad, w64.grad))
    return x, w, gy, res[0], res[1]


def _check(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    print("%s: max err %.3g, max err / bound %.3g" % (name, err.max().item(), (err / (bound + 1e-30)).max().item()))
    assert got.shape == ref.shape
    assert bool((err <= 1e-5 * bound + 1e-30).all()), "%s: max err %.3g" % (name, err.max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_s2_wgrad_and_dgrad_match_float64(geo):
    """ops.conv3d_s2_region_wgrad and conv3d_s2_region_dgrad against float64 F.conv3d autograd on the CPU: each
    element within 1e-5 x the same sum over absolute values (+ 1e-30) -- test_region_train_bwd.py's criterion."""
    from mvs_amd import ops
    b, dims, pad_lo, out = geo
    x, w, gy, (_, gx64, gw64), (_, gxa, gwa) = _reference(geo, 7 + sum(dims))
    gy_cl = gy.to(DEV).permute(0, 2, 3, 4, 1).contiguous()
    gw = ops.conv3d_s2_region_wgrad(x.to(DEV), gy_cl, pad_lo)
    gx = ops.conv3d_s2_region_dgrad(gy_cl, w.to(DEV), dims, pad_lo)
    assert gx.is_contiguous() and tuple(gx.shape) == (b, 32) + dims
    _check("gw %s" % (geo,), gw, gw64, gwa)
    _check("gx %s" % (geo,), gx, gx64, gxa)


def _impulse_voxels(geo):
    b, dims, pad_lo, out = geo
    return ((0, (0, 0, 0)), (b - 1, tuple(o - 1 for o in out)), (0, (1, 2, 10)))   # low corner, high corner, interior


@pytest.mark.gpu
def test_s2_wgrad_tap_impulses_exact():
    """One nonzero of gy (1.5 at (b, o, co)) against one of x (-2.25 at (b, ci, 2 o - pad_lo + t)), for each of
    the 27 taps, an output voxel at the low corner, the high corner and inside the box, co in each of the
    three splits: dw[co, ci, t] is exactly -3.375 and every other entry exactly 0 (a tap off the volume has no
    x to meet: all 0).  Every tap is inside the volume for at least one of the voxels."""
    from mvs_amd.ops import conv3d_s2_region_wgrad
    B, dims, pad_lo, out = IMPULSE_GEO
    seen = set()
    for corner, (b, o) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for t in range(27):
            tap = (t // 9, (t // 3) % 3, t % 3)
            co = (3, 20, 100)[(t + corner) % 3] + (t % 5)     # < 16, 16-47, >= 48
            ci = (7 * t + 11 * corner) % 32
            i = tuple(2 * oo - p + tt for oo, p, tt in zip(o, pad_lo, tap))
            inside = all(0 <= ii < d for ii, d in zip(i, dims))
            x = torch.zeros((B, 32) + dims, device=DEV)
            gy = torch.zeros((B,) + out + (112,), device=DEV)
            gy[b, o[0], o[1], o[2], co] = 1.5
            want = torch.zeros(112, 32, 3, 3, 3, device=DEV)
            if inside:
                x[b, ci, i[0], i[1], i[2]] = -2.25
                want[co, ci, tap[0], tap[1], tap[2]] = -3.375
                seen.add((t, co < 16, co >= 48))
            dw = conv3d_s2_region_wgrad(x, gy, pad_lo)
            assert torch.equal(dw, want), (corner, t, dw.nonzero().tolist())
    assert {t for t, _, _ in seen} == set(range(27))


@pytest.mark.gpu
def test_s2_dgrad_impulses_exact():
    """gy = 1.0 at one (b, o, co) with a random w: gx[b, :, 2 o - pad_lo + t] is bit-equal to w[co, :, t] for the
    taps inside the volume and gx is exactly 0 elsewhere; low corner, high corner, interior."""
    from mvs_amd.ops import conv3d_s2_region_dgrad
    B, dims, pad_lo, out = IMPULSE_GEO
    w = torch.randn(112, 32, 3, 3, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    for corner, (b, o) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for co in (5 + corner, 30 + corner, 111 - corner):
            gy = torch.zeros((B,) + out + (112,), device=DEV)
            gy[b, o[0], o[1], o[2], co] = 1.0
            want = torch.zeros((B, 32) + dims, device=DEV)
            hit = 0
            for t in range(27):
                tap = (t // 9, (t // 3) % 3, t % 3)
                i = tuple(2 * oo - p + tt for oo, p, tt in zip(o, pad_lo, tap))
                if all(0 <= ii < d for ii, d in zip(i, dims)):
                    want[b, :, i[0], i[1], i[2]] = w[co, :, tap[0], tap[1], tap[2]]
                    hit += 1
            assert hit >= 8
            gx = conv3d_s2_region_dgrad(gy, w, dims, pad_lo)
            assert torch.equal(gx, want), (corner, co, (gx != want).nonzero()[:4].tolist())


@pytest.mark.gpu
def test_s2_wgrad_reproducible_whatever_the_workspace_held():
    import ctypes
    from mvs_amd import _lib
    from mvs_amd.ops import conv3d_s2_region_wgrad
    B, dims, pad_lo, out = 2, (12, 14, 45), (1, 2, 5), (7, 8, 25)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((B, 32) + dims, device=DEV, generator=g)
    gy = torch.randn((B,) + out + (112,), device=DEV, generator=g)
    a = conv3d_s2_region_wgrad(x, gy, pad_lo)
    assert torch.equal(a, conv3d_s2_region_wgrad(x, gy, pad_lo))
    nbytes = _lib.load().mvs_conv3d_s2_region_wgrad_workspace_bytes(B, (ctypes.c_int * 3)(*dims),
                                                                    (ctypes.c_int * 3)(*out))
    assert nbytes > 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full((2 * nbytes // 4,), float("nan"), device=DEV)   # the next workspace comes out of this block
    torch.cuda.synchronize()
    del poison
    again = conv3d_s2_region_wgrad(x, gy, pad_lo)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(a, again)


def _live_s2_geometry(n):
    """(R2, pad, pad_lo, out_size) of the stacked stride-2 layer at the live geometry of a volume of extent n."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    pad, _ = pad_outpad(*n)
    M = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    R2 = _grow(M, n, 2)
    pl = tuple(max(2 * lo - p, 0) - (2 * lo - p) for (lo, _), p in zip(R2, pad))
    return R2, pad, pl, tuple(hi - lo + 1 for lo, hi in R2)


def _count_calls(monkeypatch):
    from mvs_amd import ops
    calls = []
    for name in ("conv3d_s2_region_wgrad", "conv3d_s2_region_dgrad"):
        fn = getattr(ops, name, None)

        def counted(*a, _fn=fn, _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, counted, raising=False)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("fwd", [None, "s2"])
def test_s2_box_autograd_with_hip_backward(monkeypatch, fwd):
    """region_train.s2_box at the live geometry of a (24, 20, 26) volume, B = 2, MVS_TRAIN_S2_BWD=hip: y, gx and
    gw within the float64 criterion, each new op called exactly once; forward on the tap GEMMs (switch unset)
    and on the HIP region kernel (MVS_TRAIN_REGION_FWD=s2)."""
    from mvs_amd import region_train
    monkeypatch.setenv("MVS_TRAIN_S2_BWD", "hip")
    if fwd is None:
        monkeypatch.delenv("MVS_TRAIN_REGION_FWD", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_REGION_FWD", fwd)
    n = (24, 20, 26)
    R2, pad, pl, size = _live_s2_geometry(n)
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _reference((2, n, pl, size), 5)
    calls = _count_calls(monkeypatch)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    assert region_train.s2_bwd_enabled(xg) and region_train.enabled(xg, "s2") is (fwd == "s2")
    y = region_train.s2_box(xg, wg, R2, pad, pl, region_train.S2_SPLITS)
    (y * gy.to(DEV)).sum().backward()
    assert sorted(calls) == ["conv3d_s2_region_dgrad", "conv3d_s2_region_wgrad"], calls
    assert xg.grad.is_contiguous()
    _check("y", y.detach(), y64, ya)
    _check("gx", xg.grad, gx64, gxa)
    _check("gw", wg.grad, gw64, gwa)


@pytest.mark.gpu
def test_default_s2_path_is_the_tap_gemms(monkeypatch):
    """Both switches unset: _conv_s2_region under autograd calls neither new op and its y, gx and gw are bit-equal
    to tap_gemm.conv3d_box's."""
    from mvs_amd import regions, tap_gemm
    monkeypatch.delenv("MVS_TRAIN_S2_BWD", raising=False)
    monkeypatch.delenv("MVS_TRAIN_REGION_FWD", raising=False)
    n = (24, 20, 26)
    R2, pad, pl, size = _live_s2_geometry(n)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, *n, generator=g)
    w = torch.randn(112, 32, 3, 3, 3, generator=g) * 0.05
    gy = torch.randn(2, 112, *size, generator=g).to(DEV)
    calls = _count_calls(monkeypatch)
    res = []
    for fn in (lambda a, b: regions._conv_s2_region(a, b, R2, pad, splits=(16, 32, 64)),
               lambda a, b: tap_gemm.conv3d_box(a, b, 2, pl, size)):
        xs = [t.clone().to(DEV).requires_grad_(True) for t in (x, w)]
        y = fn(*xs)
        (y * gy).sum().backward()
        res.append([y.detach()] + [t.grad for t in xs])
    assert calls == []
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


@pytest.mark.gpu
def test_regulariser_chain_with_hip_s2_backward(monkeypatch):
    """CostVolumeReg in train mode under autograd with the stride-2 layers' HIP backward (forward switch at its
    default), loss sum(P * Wr) on a random cost volume (B = 2, (16, 20, 24)): every parameter's gradient and the
    cost volume's, relative L2 to float64 forward_full <= 2 x the CPU fp32 forward_full gradient's + 1e-5
    (test_gpu_train.py's criterion)."""
    from conftest import record_parity
    from weights import deterministic_state_dict
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    monkeypatch.setenv("MVS_TRAIN_S2_BWD", "hip")
    monkeypatch.delenv("MVS_TRAIN_REGION_FWD", raising=False)
    B, n = 2, (16, 20, 24)
    pad, outpad = pad_outpad(*n)
    reg = CostVolumeReg(pad=pad, outpad=outpad)
    reg.load_state_dict(deterministic_state_dict(reg.state_dict(), seed=99))
    reg.train()
    reg_c, reg_d, reg_g = copy.deepcopy(reg), copy.deepcopy(reg).double(), copy.deepcopy(reg).to(DEV)
    g = torch.Generator().manual_seed(41)
    cv = torch.rand(B, 32, *n, generator=g)
    wr = torch.randn(B, 1, *n, generator=g)

    calls = _count_calls(monkeypatch)
    cv_g = cv.to(DEV).requires_grad_(True)
    cv_c, cv_d = cv.clone().requires_grad_(True), cv.double().requires_grad_(True)
    assert reg_g.live_autograd_ok(cv_g)
    (reg_g(cv_g) * wr.to(DEV)).sum().backward()
    assert sorted(calls) == ["conv3d_s2_region_dgrad", "conv3d_s2_region_wgrad"], calls
    (reg_c.forward_full(cv_c) * wr).sum().backward()
    (reg_d.forward_full(cv_d) * wr.double()).sum().backward()

    pg, pc, pd = (dict(m.named_parameters()) for m in (reg_g, reg_c, reg_d))
    assert all((pg[k].grad is None) == (pd[k].grad is None) for k in pd)
    errs = {k: (_rel(pg[k].grad.cpu(), pd[k].grad), _rel(pc[k].grad, pd[k].grad)) for k in sorted(pd)
            if pd[k].grad is not None}
    assert {"conv_1_0.weight", "conv_2_0.weight", "conv_3_0.weight"} <= set(errs)
    errs["cost_volume"] = (_rel(cv_g.grad.cpu(), cv_d.grad), _rel(cv_c.grad, cv_d.grad))
    record_parity("region_s2_hip_backward_chain_grads", grad_rel_l2_gpu_vs_f64_max=max(v[0] for v in errs.values()),
                  grad_rel_l2_cpu_vs_f64_max=max(v[1] for v in errs.values()),
                  per_parameter={k: [float(a), float(b)] for k, (a, b) in errs.items()})
    for name, (e_g, e_c) in errs.items():
        print("%s: GPU %.3g, CPU fp32 %.3g" % (name, e_g, e_c))
    for name, (e_g, e_c) in errs.items():
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
