"""GPU: the stride-1 region convolutions' HIP backward under autograd (MVS_TRAIN_REGION_BWD=s1;
mvs_amd/region_train.py _S1Valid: the input gradient on the forward's region kernel in its adjoint
geometry, the weight gradient on csrc/conv3d_region_wgrad.hip) against float64 torch autograd, the weight
gradient's tap / voxel / channel placement on exact impulses, its bit-reproducibility whatever the
workspace held, the default (tap-GEMM) backward unchanged, and the regulariser's whole autograd chain.
(One pass of the weight gradient's tile loop throughout; the multi-pass cases: test_region_train_multipass.py.)"""
import copy

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

# (B, Lz, Ly, Lx) of the padded crop: one output voxel (K = 1); 17 outputs along x (one past a 16-row MFMA
# block); odd extents across tile edges with several samples; deeper than wide
SHAPES = [(1, 3, 3, 3), (2, 4, 5, 19), (3, 6, 7, 37), (1, 11, 6, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("c", [16, 32, 64])
def test_s1_hip_backward_matches_float64(monkeypatch, c, shape):
    """y, gx and gw of region_train.s1_valid with the HIP backward against F.conv3d in float64 on the CPU:
    each within 1e-5 x the same sum over absolute values (+ 1e-30), elementwise -- the criterion of
    test_narrow_train.py::test_narrow_conv_autograd_matches_float64."""
    from mvs_amd import region_train
    monkeypatch.setenv("MVS_TRAIN_REGION_BWD", "s1")
    assert region_train.bwd_enabled("s1", c)
    b, lz, ly, lx = shape
    g = torch.Generator().manual_seed(c * 100 + sum(shape))
    x = torch.randn(b, c, lz, ly, lx, generator=g)
    wt = torch.randn(c, c, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, c, lz - 2, ly - 2, lx - 2, generator=g)
    xg, wg = x.to(DEV).requires_grad_(True), wt.to(DEV).requires_grad_(True)
    y = region_train.s1_valid(xg, wg)
    (y * gy.to(DEV)).sum().backward()
    x64, w64 = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64)
    (y64 * gy.double()).sum().backward()
    xa, wa = x.double().abs().requires_grad_(True), wt.double().abs().requires_grad_(True)
    ya = F.conv3d(xa, wa)
    (ya * gy.double().abs()).sum().backward()
    assert y.shape == y64.shape and xg.grad.shape == x.shape and wg.grad.shape == wt.shape
    for name, got, ref, bound in (("y", y.detach(), y64.detach(), ya.detach()), ("gx", xg.grad, x64.grad, xa.grad),
                                  ("gw", wg.grad, w64.grad, wa.grad)):
        err = (got.double().cpu() - ref).abs()
        print("%s C=%d %s: max err %.3g, max err / bound %.3g" % (name, c, shape, err.max().item(),
                                                                    (err / (bound + 1e-30)).max().item()))
        assert bool((err <= 1e-5 * bound + 1e-30).all()), "%s: max err %.3g" % (name, err.max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("c", [16, 64])
def test_region_wgrad_tap_impulses_exact(c):
    """One nonzero of gy (1.5 at (b, o, co)) against one of x (-2.25 at (b, o + t, ci)), for each of the 27
    taps and an output voxel at the low and at the high corner of the box: dw[co, ci, t] is exactly -3.375
    and every other entry exactly 0."""
    from mvs_amd.ops import conv3d_region_wgrad
    B, L = 2, (6, 9, 21)   # outputs (4, 7, 19): two tiles along x, rows past one tile for every C
    O = tuple(d - 2 for d in L)
    for corner, (b, o) in enumerate(((0, (0, 0, 0)), (B - 1, tuple(d - 1 for d in O)))):
        for t in range(27):
            tz, ty, tx = t // 9, (t // 3) % 3, t % 3
            co, ci = (5 * t + 3 + corner) % c, (7 * t + 11 * corner) % c
            x = torch.zeros((B,) + L + (c,), device=DEV)
            gy = torch.zeros((B,) + O + (c,), device=DEV)
            gy[b, o[0], o[1], o[2], co] = 1.5
            x[b, o[0] + tz, o[1] + ty, o[2] + tx, ci] = -2.25
            dw = conv3d_region_wgrad(x, gy)
            want = torch.zeros(c, c, 3, 3, 3, device=DEV)
            want[co, ci, tz, ty, tx] = -3.375
            assert torch.equal(dw, want), (corner, t, dw.nonzero().tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("c", [16, 32, 64])
def test_region_wgrad_reproducible_whatever_the_workspace_held(c):
    from mvs_amd import _lib
    from mvs_amd.ops import conv3d_region_wgrad
    B, L = 2, (7, 12, 40)
    g = torch.Generator(device=DEV).manual_seed(c)
    x = torch.randn((B,) + L + (c,), device=DEV, generator=g)
    gy = torch.randn((B,) + tuple(d - 2 for d in L) + (c,), device=DEV, generator=g)
    a = conv3d_region_wgrad(x, gy)
    assert torch.equal(a, conv3d_region_wgrad(x, gy))
    import ctypes
    nbytes = _lib.load().mvs_conv3d_region_wgrad_workspace_bytes(B, c, (ctypes.c_int * 3)(*L))
    assert nbytes > 0
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full((2 * nbytes // 4,), float("nan"), device=DEV)   # the next workspace comes out of this block
    torch.cuda.synchronize()
    del poison
    again = conv3d_region_wgrad(x, gy)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(a, again)


@pytest.mark.gpu
def test_default_backward_is_the_tap_gemms(monkeypatch):
    """Switch unset: s1_valid's gradients are bit-equal to tap_gemm.conv3d's (the same backward on the same
    saved operands), at the stride-1 live geometry of a (24, 20, 26) volume, C = 32."""
    from mvs_amd import region_train, tap_gemm
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    n = (24, 20, 26)
    pad, _ = pad_outpad(*n)
    M = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    R1 = _grow(M, n, 1)
    g = torch.Generator().manual_seed(5)
    xin = torch.randn(2, 32, *[hi - lo + 3 for lo, hi in R1], generator=g)
    w1 = torch.randn(32, 32, 3, 3, 3, generator=g) * 0.05
    gy, grads = None, []
    for fn in (region_train.s1_valid, lambda a, b: tap_gemm.conv3d(a, b, 1, 0)):
        xs = [t.clone().to(DEV).requires_grad_(True) for t in (xin, w1)]
        y = fn(*xs)
        if gy is None:
            gy = torch.randn(y.shape, generator=g).to(DEV)
        (y * gy).sum().backward()
        grads.append([t.grad for t in xs])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


@pytest.mark.gpu
def test_regulariser_chain_with_hip_s1_backward(monkeypatch):
    """CostVolumeReg in train mode under autograd with the stride-1 layers' HIP backward, loss sum(P * Wr) on a
    random cost volume (B = 2, (16, 20, 24)): every parameter's gradient, relative L2 to float64 forward_full
    <= 2 x the CPU fp32 forward_full gradient's + 1e-5 (test_gpu_train.py's criterion)."""
    from conftest import record_parity
    from weights import deterministic_state_dict
    from mvs_amd import ops
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    monkeypatch.setenv("MVS_TRAIN_REGION_BWD", "s1")
    B, n = 2, (16, 20, 24)
    pad, outpad = pad_outpad(*n)
    reg = CostVolumeReg(pad=pad, outpad=outpad)
    reg.load_state_dict(deterministic_state_dict(reg.state_dict(), seed=99))
    reg.train()
    reg_c, reg_d, reg_g = copy.deepcopy(reg), copy.deepcopy(reg).double(), copy.deepcopy(reg).to(DEV)
    g = torch.Generator().manual_seed(41)
    cv = torch.rand(B, 32, *n, generator=g)
    wr = torch.randn(B, 1, *n, generator=g)

    calls = []
    wgrad = ops.conv3d_region_wgrad

    def counted(x_cl, gy_cl):
        calls.append(x_cl.shape[-1])
        return wgrad(x_cl, gy_cl)
    monkeypatch.setattr(ops, "conv3d_region_wgrad", counted)
    cv_g = cv.to(DEV)
    assert reg_g.live_autograd_ok(cv_g)
    (reg_g(cv_g) * wr.to(DEV)).sum().backward()
    assert sorted(calls) == [16, 32, 64], calls   # conv_1_1, conv_2_1, conv_3_1 took the HIP backward
    (reg_c.forward_full(cv) * wr).sum().backward()
    (reg_d.forward_full(cv.double()) * wr.double()).sum().backward()

    pg, pc, pd = (dict(m.named_parameters()) for m in (reg_g, reg_c, reg_d))
    assert all((pg[k].grad is None) == (pd[k].grad is None) for k in pd)
    errs = {k: (_rel(pg[k].grad.cpu(), pd[k].grad), _rel(pc[k].grad, pd[k].grad)) for k in sorted(pd)
            if pd[k].grad is not None}
    assert {"conv_1_1.weight", "conv_2_1.weight", "conv_3_1.weight"} <= set(errs)
    record_parity("region_s1_hip_backward_chain_grads", grad_rel_l2_gpu_vs_f64_max=max(v[0] for v in errs.values()),
                  grad_rel_l2_cpu_vs_f64_max=max(v[1] for v in errs.values()),
                  per_parameter={k: [float(a), float(b)] for k, (a, b) in errs.items()})
    for name, (e_g, e_c) in errs.items():
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
