"""MVS_TRAIN_BN: the switch (CPU), and on the GPU the routing of CostVolumeReg.forward_live_train's ten BatchNorm + ReLU
sites onto bn_train.bn_relu_train, the default path bit-equal to the torch sequence it had before the switch
existed, the regulariser chain against float64 CPU autograd, and peak memory.

The geometry is region_cases.GEOMETRIES' (20, 32, 40) with B = 2."""
import copy
import functools

import pytest
import torch

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
OTHER_SWITCHES = ("MVS_TRAIN_DECONV1", "MVS_TRAIN_T2_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_REGION_BWD")
ALL_FIVE = ("MVS_TRAIN_BN",) + OTHER_SWITCHES
CHAIN_B, CHAIN_N = 2, (20, 32, 40)


class _OnGpu:
    is_cuda, dtype = True, torch.float32


def _clear(monkeypatch):
    for name in ALL_FIVE + ("MVS_TRAIN_REGION_FWD", "MVS_TRAIN_LIVE"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("torch", False), ("hip", True), ("HIP", False),
                                      ("1", False), ("hip,torch", False), ("junk", False)])
def test_bn_switch(monkeypatch, value, on):
    """MVS_TRAIN_BN=hip alone turns the path on (read through a stand-in with a GPU tensor's attributes); anything
    else, junk included, is the torch path, as with the neighbouring switches.  It changes none of their answers."""
    from mvs_amd import bn_train, region_train
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv("MVS_TRAIN_BN", value)
    assert bn_train.enabled(_OnGpu()) is on
    assert not bn_train.enabled(torch.zeros(1))            # a CPU tensor: never

    class Half:
        is_cuda, dtype = True, torch.float16
    assert not bn_train.enabled(Half())
    with torch.no_grad():
        assert not bn_train.enabled(_OnGpu())
    assert not region_train.d1_enabled(_OnGpu()) and not region_train.s2_bwd_enabled(_OnGpu())
    assert not region_train.t2_bwd_enabled(_OnGpu()) and not region_train.bwd_enabled("s1")
    assert region_train.enabled(_OnGpu(), "s1") and region_train.enabled(_OnGpu(), "t2")
    assert not region_train.enabled(_OnGpu(), "s2")


def test_other_switches_do_not_enable_bn(monkeypatch):
    from mvs_amd import bn_train
    _clear(monkeypatch)
    for name in OTHER_SWITCHES + ("MVS_TRAIN_REGION_FWD",):
        for v in ("hip", "taps", "s1", "bn", "torch", "s1,t2"):
            monkeypatch.setenv(name, v)
            assert not bn_train.enabled(_OnGpu()), (name, v)
        monkeypatch.delenv(name, raising=False)
    for name in OTHER_SWITCHES + ("MVS_TRAIN_REGION_FWD",):       # all on at once
        monkeypatch.setenv(name, "hip")
    assert not bn_train.enabled(_OnGpu())


def _regulariser(n):
    from weights import deterministic_state_dict
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    pad, outpad = pad_outpad(*n)
    reg = CostVolumeReg(pad=pad, outpad=outpad)
    reg.load_state_dict(deterministic_state_dict(reg.state_dict(), seed=99))
    return reg.train()


def _before_the_switch(self, cv):
    """CostVolumeReg.forward_live_train's torch sequence as it was before MVS_TRAIN_BN existed, from the same
    functions (bn_sums._sums / _bn_train / _apply_bn / _bn_constant / _border_class_sums, regions.*)."""
    from mvs_amd.bn_sums import _apply_bn, _bn_constant, _bn_train, _border_class_sums, _sums
    from mvs_amd.regions import _conv_s1_region, _conv_s2_region, _crop_pad, _grow, _tconv_region, live_regions
    from mvs_amd.regulariser import _narrow_conv
    act = lambda y, bn: self.ReLU(_apply_bn(y, *bn))
    n = tuple(cv.shape[2:5])
    full, M = live_regions(n, self.pad)[:2]
    R1, R2 = _grow(M, n, 1), _grow(M, n, 2)
    bsz = cv.shape[0]
    count = bsz * n[0] * n[1] * n[2]
    y0 = _narrow_conv(self.conv_0_0, cv)
    y0 = act(y0, _bn_train(self.BN_0, *_sums(y0), count))
    stage = []
    convs_a = ((self.conv_1_0, self.BN_1), (self.conv_2_0, self.BN_2), (self.conv_3_0, self.BN_3))
    zs = _conv_s2_region(cv, torch.cat([c.weight for c, _ in convs_a], 0), R2, self.pad,
                         splits=tuple(c.weight.shape[0] for c, _ in convs_a))
    zs = zs.split([c.weight.shape[0] for c, _ in convs_a], 1)
    for z, (conv_a, bn) in zip(zs, convs_a):
        p = _bn_train(bn, *_sums(z), count)
        stage.append((act(z, p), _bn_constant(p)))
    lv = []
    for (y, a), conv_b, bn in zip(stage, (self.conv_1_1, self.conv_2_1, self.conv_3_1),
                                  (self.BN_1, self.BN_2, self.BN_3)):
        z = _conv_s1_region(y, R2, conv_b.weight, R1, n)
        s1, s2 = _sums(z)
        c1, c2 = _border_class_sums(conv_b.weight, a, R1, n, bsz)
        p = _bn_train(bn, s1 + c1, s2 + c2, count)
        lv.append(_crop_pad(act(z, p), R1, M, n))
    y1, y2, y3 = lv
    z = _tconv_region(y3, M, self.deconv_3_0.weight, full, self.pad, n)
    y3 = act(_crop_pad(z, full, M, n), _bn_train(self.BN_2, *_sums(z), count))
    z = _tconv_region(y3 + y2, M, self.deconv_2_0.weight, full, self.pad, n)
    y2 = act(_crop_pad(z, full, M, n), _bn_train(self.BN_1, *_sums(z), count))
    z = _tconv_region(y2 + y1, M, self.deconv_1_0.weight, full, self.pad)
    z = act(z, _bn_train(self.BN_0, *_sums(z), count)) + y0
    return self.Norm(_narrow_conv(self.conv_out, z))


def _step(reg, cv, wr, forward):
    cv = cv.detach().clone().requires_grad_(True)
    out = forward(reg, cv)
    (out * wr).sum().backward()
    grads = {k: v.grad for k, v in reg.named_parameters()}
    return out.detach(), cv.grad, grads, {k: v.detach().clone() for k, v in reg.named_buffers()}


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert set(a[2]) == set(b[2]) and set(a[3]) == set(b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def _refuse_the_new_op(monkeypatch):
    from mvs_amd import bn_train

    def refuse(*a, **k):
        raise AssertionError("bn_relu_train was called")
    monkeypatch.setattr(bn_train, "bn_relu_train", refuse)
    monkeypatch.setattr(bn_train._BnReluTrain, "apply", refuse)


@pytest.mark.parametrize("value", [None, "hip"])
def test_cpu_forward_live_train_is_the_torch_sequence(monkeypatch, value):
    """On the CPU the switch never applies: forward_live_train's outputs, gradients and running statistics are
    bit-equal to the torch sequence from before the switch, whatever its value, and the new op is never called."""
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv("MVS_TRAIN_BN", value)
    _refuse_the_new_op(monkeypatch)
    n = (5, 6, 6)
    reg = _regulariser(n)
    g = torch.Generator().manual_seed(4)
    cv, wr = torch.rand(2, 32, *n, generator=g), torch.randn(2, 1, *n, generator=g)
    _same(_step(copy.deepcopy(reg), cv, wr, lambda m, x: m.forward_live_train(x)),
          _step(copy.deepcopy(reg), cv, wr, _before_the_switch))


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """The regulariser, its inputs, and the float64 / CPU fp32 forward_full gradients and running statistics:
    computed once."""
    reg = _regulariser(CHAIN_N)
    g = torch.Generator().manual_seed(41)
    cv = torch.rand(CHAIN_B, 32, *CHAIN_N, generator=g)
    wr = torch.randn(CHAIN_B, 1, *CHAIN_N, generator=g)
    full = lambda m, x: m.forward_full(x)
    _, cvg_c, pc, bc = _step(copy.deepcopy(reg), cv, wr, full)
    _, cvg_d, pd, bd = _step(copy.deepcopy(reg).double(), cv.double(), wr.double(), full)
    return reg, cv, wr, pc, pd, cvg_c, cvg_d, bc, bd


def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


@pytest.mark.gpu
def test_switch_on_routes_all_ten_sites(monkeypatch):
    """MVS_TRAIN_BN=hip: bn_sums._sums and _apply_bn raise if called, forward_live_train + backward completes, and
    bn_relu_train ran ten times (lines BN_0, BN_1, BN_2, BN_3, BN_1, BN_2, BN_3, BN_2, BN_1, BN_0)."""
    from mvs_amd import bn_sums, bn_train, regulariser
    _clear(monkeypatch)
    monkeypatch.setenv("MVS_TRAIN_BN", "hip")

    def refuse(*a, **k):
        raise AssertionError("a torch BN pass was called")
    for mod in (bn_sums, regulariser):
        monkeypatch.setattr(mod, "_sums", refuse)
        monkeypatch.setattr(mod, "_apply_bn", refuse)
    calls = []
    real = bn_train.bn_relu_train

    def counted(z, box, bn, extra, count):
        calls.append((z.shape[1], box is not None, extra is not None))
        return real(z, box, bn, extra, count)
    monkeypatch.setattr(bn_train, "bn_relu_train", counted)
    reg, cv, wr = _chain_reference()[:3]
    reg_g = copy.deepcopy(reg).to(DEV)
    cv_g = cv.to(DEV).requires_grad_(True)
    assert reg_g.live_autograd_ok(cv_g) and bn_train.enabled(cv_g)
    (reg_g(cv_g) * wr.to(DEV)).sum().backward()
    assert calls == [(8, False, False), (16, False, False), (32, False, False), (64, False, False),
                     (16, True, True), (32, True, True), (64, True, True), (32, True, False), (16, True, False),
                     (8, False, False)], calls
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in reg_g.parameters())
    assert all(int(bn.num_batches_tracked) == k for bn, k in zip(reg_g._bns, (2, 3, 3, 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("value", [None, "torch", ""])
def test_switch_off_is_the_torch_sequence(monkeypatch, value):
    """The switch off: the new op raises if called, and outputs, every gradient and every running statistic are
    bit-equal to the torch sequence from before the switch."""
    _clear(monkeypatch)
    if value is not None:
        monkeypatch.setenv("MVS_TRAIN_BN", value)
    _refuse_the_new_op(monkeypatch)
    reg, cv, wr = _chain_reference()[:3]
    cv_g, wr_g = cv.to(DEV), wr.to(DEV)
    probe = cv_g.clone().requires_grad_(True)
    assert copy.deepcopy(reg).to(DEV).live_autograd_ok(probe)
    _same(_step(copy.deepcopy(reg).to(DEV), cv_g, wr_g, lambda m, x: m(x)),
          _step(copy.deepcopy(reg).to(DEV), cv_g, wr_g, _before_the_switch))


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [("MVS_TRAIN_BN",), ALL_FIVE])
def test_regulariser_chain_with_hip_bn(monkeypatch, switches):
    """CostVolumeReg in train mode under autograd with the BN + ReLU sites on the HIP kernels -- alone, then with
    the four other training switches as well -- loss sum(P * Wr) on a random cost volume: every parameter's gradient,
    the cost volume's and every BN running statistic, relative L2 to float64 forward_full on the CPU <= 2 x the CPU
    fp32 forward_full's + 1e-5 (test_regulariser_chain_with_hip_deconv1's bound)."""
    from conftest import record_parity
    _clear(monkeypatch)
    for name in switches:
        monkeypatch.setenv(name, "s1" if name == "MVS_TRAIN_REGION_BWD" else "hip")
    reg, cv, wr, pc, pd, cvg_c, cvg_d, bc, bd = _chain_reference()
    reg_g = copy.deepcopy(reg).to(DEV)
    _, cvg_g, pg, bg = _step(reg_g, cv.to(DEV), wr.to(DEV), lambda m, x: m(x))
    assert all((pg[k] is None) == (pd[k] is None) for k in pd)
    errs = {k: (_rel(pg[k].cpu(), pd[k]), _rel(pc[k], pd[k])) for k in sorted(pd) if pd[k] is not None}
    assert {"BN_0.weight", "BN_3.bias", "conv_3_1.weight", "deconv_1_0.weight"} <= set(errs)
    errs["cost_volume"] = (_rel(cvg_g.cpu(), cvg_d), _rel(cvg_c, cvg_d))
    for k in sorted(bd):
        if k.endswith("num_batches_tracked"):
            assert torch.equal(bg[k].cpu(), bd[k]), k
        else:
            errs[k] = (_rel(bg[k].cpu(), bd[k]), _rel(bc[k], bd[k]))
    record_parity("bn_train_hip_chain_%d" % len(switches),
                  rel_l2_gpu_vs_f64_max=max(v[0] for v in errs.values()),
                  rel_l2_cpu_vs_f64_max=max(v[1] for v in errs.values()),
                  per_tensor={k: [float(a), float(b)] for k, (a, b) in errs.items()})
    worst = max(errs, key=lambda k: errs[k][0] / (2.0 * errs[k][1] + 1e-5))
    print("worst tensor %s: GPU %.3g, CPU fp32 %.3g, bound %.3g"
          % (worst, errs[worst][0], errs[worst][1], 2.0 * errs[worst][1] + 1e-5))
    for name, (e_g, e_c) in errs.items():
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)


@pytest.mark.gpu
def test_peak_memory_not_higher_with_the_switch(monkeypatch):
    """torch.cuda.max_memory_allocated of one forward + backward of the regulariser: with the switch on it is not
    higher than with it off (the fused node keeps z and per-channel vectors, the torch ops three or four full-size
    intermediates per site)."""
    reg, cv, wr = _chain_reference()[:3]
    cv_g, wr_g = cv.to(DEV), wr.to(DEV)
    peak = {}
    for value in ("torch", "hip"):
        _clear(monkeypatch)
        monkeypatch.setenv("MVS_TRAIN_BN", value)
        reg_g = copy.deepcopy(reg).to(DEV)
        for _ in range(2):   # (the first pass fills the caches of derived weights and workspaces)
            reg_g.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(DEV)
            base = torch.cuda.memory_allocated(DEV)
            _step(reg_g, cv_g, wr_g, lambda m, x: m(x))
            torch.cuda.synchronize()
            peak[value] = torch.cuda.max_memory_allocated(DEV) - base
        del reg_g
    print("peak memory above the start: torch %.1f MB, hip %.1f MB" % (peak["torch"] / 2 ** 20, peak["hip"] / 2 ** 20))
    assert peak["hip"] <= peak["torch"], peak
