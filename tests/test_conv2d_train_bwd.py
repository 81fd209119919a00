"""GPU: the 2-D convolutions' HIP backward (MVS_TRAIN_CONV2D_BWD=hip; mvs_amd/conv2d_train.py over
csrc/conv2d_bwd.hip): both gradients against float64 F.conv2d autograd on the CPU for all eight layer shapes, the
weight gradient's placement on exact impulses, its bit-reproducibility whatever the workspace held, its persistent
tile loop over several passes, the autograd routing under the switch and the untouched default, and the encoder and
refinement stacks' whole chains.

Criterion of the float64 parity (test_region_train_s2_bwd.py's _check): every element within 1e-5 x the same sum
taken over absolute values + 1e-30.  Measured maxima of err / that sum on an MI355X (the printed "max err /
bound"): MEASURED_PARITY below.

Mutation runs (scratch builds of csrc/conv2d_bwd.hip, not committed): MUTATIONS below."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

SHAPES = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (4, 32, 3, 1),
          (32, 1, 3, 1))
# (H, W) of the input.  The input gradient's tile is 8 rows x 64 columns of input pixels (stride 2: 8 rows of one
# parity x 64 columns, i.e. 16 x 64), the weight gradient's 8 x 32 output pixels: one pixel; smaller than any halo;
# one past the weight gradient's tile both ways; one past the input gradient's; two tile rows and a ragged width
S1_SIZES = ((1, 1), (2, 3), (9, 33), (9, 65), (17, 40))
# stride 2 adds both parities of H and W (the last partial output row / column, both input parities at the edge) and
# sizes one past a tile of either kernel in input pixels (16 x 64) and in output pixels
S2_SIZES = ((1, 1), (2, 3), (7, 10), (8, 9), (17, 66), (18, 65), (19, 131))
BATCHES = (1, 3)

MEASURED_PARITY = """max over sizes and batches of err / (sum over absolute values), gw / gx, MI355X (1e-5 allowed):
(3,8,3,1) 1.16e-7 / 2.44e-7   (8,8,3,1) 1.78e-7 / 2.20e-7   (8,16,5,2) 2.02e-7 / 2.92e-7   (16,16,3,1) 1.57e-7 / 2.54e-7
(16,32,5,2) 1.96e-7 / 3.34e-7   (32,32,3,1) 1.82e-7 / 3.37e-7   (4,32,3,1) 1.31e-7 / 2.17e-7   (32,1,3,1) 1.13e-7 / 2.06e-7"""
MUTATIONS = """Two scratch builds of csrc/conv2d_bwd.hip (not committed), this file run once against each on an MI355X:
A, the weight gradient's accumulators zeroed at the top of its tile loop: 1 failed, 26 passed.  The one is
  test_weight_gradient_multi_pass (gw max err 2.24e+03); every other case has at most 512 tiles, one per workgroup.
B, the sums of the odd input rows (PY = 1) of the stride-2 input gradient dropped: 5 failed, 22 passed --
  test_gradients_match_float64[8x16x5x2] and [16x32x5x2] (gx, first at n=1 2x3: 1x1 has no odd row; max err 1.84
  and 1.13), test_routing[8x16x5x2] (gx against the tap GEMMs') and test_chain[encoder-alone] and
  [encoder-all_six] (relative error 0.92 from the first weight on).  The stride-1 shapes, every gw-only test and
  the refinement chain (no stride-2 layer) pass."""


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _sizes(stride):
    return S1_SIZES if stride == 1 else S2_SIZES


@functools.lru_cache(maxsize=None)
def _reference(shape, n, hw, seed=0):
    """Inputs and the float64 CPU gradients (gx, gw), then the same sums over absolute values; computed once."""
    cin, cout, k, s = shape
    g = torch.Generator().manual_seed(1000 * n + 31 * hw[0] + hw[1] + seed + 7 * cin + cout)
    x = torch.randn(n, cin, *hw, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1
    ho, wo = ((d + 2 * (k // 2) - k) // s + 1 for d in hw)
    gy = torch.randn(n, cout, ho, wo, generator=g)
    res = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        x64, w64 = f(x).requires_grad_(True), f(w).requires_grad_(True)
        (F.conv2d(x64, w64, stride=s, padding=k // 2) * f(gy)).sum().backward()
        res.append((x64.grad, w64.grad))
    return x, w, gy, res[0], res[1]


def _check(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    ratio = (err / (bound + 1e-30)).max().item()
    print("%s: max err %.3g, max err / bound %.3g" % (name, err.max().item(), ratio))
    assert got.shape == ref.shape
    assert bool((err <= 1e-5 * bound + 1e-30).all()), "%s: max err %.3g" % (name, err.max().item())
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_gradients_match_float64(shape):
    """conv2d_wgrad and conv2d_dgrad against float64 F.conv2d autograd at every size and batch (gx of the (3, 8, 3, 1)
    layer too: the model never asks for it, the kernel computes it all the same)."""
    from mvs_amd import conv2d_train
    cin, cout, k, s = shape
    worst = {"gw": 0.0, "gx": 0.0}
    for hw in _sizes(s):
        for n in BATCHES:
            x, w, gy, (gx64, gw64), (gxa, gwa) = _reference(shape, n, hw)
            gw = conv2d_train.conv2d_wgrad(x.to(DEV), gy.to(DEV), k, s)
            gx = conv2d_train.conv2d_dgrad(gy.to(DEV), w.to(DEV), s, hw[0], hw[1])
            assert gx.is_contiguous() and tuple(gx.shape) == (n, cin) + hw
            assert gw.is_contiguous() and tuple(gw.shape) == (cout, cin, k, k)
            tag = "%s n=%d %dx%d" % (shape, n, hw[0], hw[1])
            worst["gw"] = max(worst["gw"], _check("gw " + tag, gw, gw64, gwa))
            worst["gx"] = max(worst["gx"], _check("gx " + tag, gx, gx64, gxa))
    print("MAXIMA %s: gw %.3g gx %.3g (of the 1e-5 allowed)" % (shape, worst["gw"], worst["gx"]))


IMPULSE_N, IMPULSE_HW = 2, (19, 70)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_weight_gradient_exact_impulses(shape):
    """One non-zero gy element (the low corner of image 0, the high corner of the last image, an interior pixel past
    the first tile) and one non-zero x element under tap (ky, kx) of it: gw has the single entry
    [co][ci][ky][kx] = the product, bit for bit (1.5 * -2.25 is exact), for every tap whose input pixel is inside
    the image.  For the others (they read padding) x is put at pixel (0, 0) instead: the only entry allowed is the
    tap, if any, that reaches (0, 0) from the spot."""
    from mvs_amd import conv2d_train
    cin, cout, k, s = shape
    n, (h, wd) = IMPULSE_N, IMPULSE_HW
    ho, wo = ((d + 2 * (k // 2) - k) // s + 1 for d in (h, wd))
    spots = ((0, 0, 0), (n - 1, ho - 1, wo - 1), (0, min(9, ho - 1), min(33, wo - 1)))
    hits = 0
    for b, oy, ox in spots:
        for t in range(k * k):
            ky, kx = t // k, t % k
            iy, ix = oy * s + ky - k // 2, ox * s + kx - k // 2
            ci, co = t % cin, (3 * t + 1) % cout
            x = torch.zeros(n, cin, h, wd, device=DEV)
            gy = torch.zeros(n, cout, ho, wo, device=DEV)
            gy[b, co, oy, ox] = 1.5
            inside = 0 <= iy < h and 0 <= ix < wd
            x[b, ci, iy if inside else 0, ix if inside else 0] = -2.25
            gw = conv2d_train.conv2d_wgrad(x, gy, k, s)
            want = torch.zeros(cout, cin, k, k)
            if inside:
                want[co, ci, ky, kx] = 1.5 * -2.25
                hits += 1
            else:
                # x sits at (0, 0): the tap (if any) that reaches it from (oy, ox) is the only entry
                qy, qx = 0 - oy * s + k // 2, 0 - ox * s + k // 2
                if 0 <= qy < k and 0 <= qx < k:
                    want[co, ci, qy, qx] = 1.5 * -2.25
            assert torch.equal(gw.cpu(), want), (shape, (b, oy, ox), (ky, kx), gw.cpu().nonzero().tolist())
    # the interior spot has every tap, the low corner those with ky, kx >= k // 2, the high corner at least one
    assert hits >= k * k + (k - k // 2) ** 2 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n,hw", [((8, 8, 3, 1), 3, (40, 100)), ((16, 32, 5, 2), 2, (37, 131)),
                                        ((3, 8, 3, 1), 1, (17, 40)), ((32, 1, 3, 1), 2, (9, 65))], ids=_id)
def test_weight_gradient_ignores_the_workspace(shape, n, hw):
    """gw is bit-equal after a NaN-filled workspace and after a zeroed one (and equal to the op's own)."""
    from mvs_amd import _lib, conv2d_train
    cin, cout, k, s = shape
    x, w, gy, _, _ = _reference(shape, n, hw, seed=5)
    xg, gyg = x.to(DEV), gy.to(DEV)
    nbytes = _lib.load().mvs_conv2d_wgrad_workspace_bytes(n, cin, cout, hw[0], hw[1], k, s)
    assert nbytes > 0
    nan = torch.full((nbytes // 4,), float("nan"), device=DEV)
    zero = torch.zeros(nbytes // 4, device=DEV)
    a = conv2d_train._wgrad(xg, gyg, k, s, nan)
    b = conv2d_train._wgrad(xg, gyg, k, s, zero)
    c = conv2d_train.conv2d_wgrad(xg, gyg, k, s)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not bool(torch.isnan(nan).all())   # the slots were written


@pytest.mark.gpu
def test_weight_gradient_multi_pass():
    """A full-resolution image pair of the 3 -> 8 layer: every persistent workgroup walks four or five tiles, the
    last row and column of tiles ragged -- asserted through the plan query, so the case cannot silently become
    single-pass."""
    from mvs_amd import conv2d_train
    shape = (3, 8, 3, 1)
    cin, cout, k, s = shape
    n, hw = 2, (500, 637)
    tiles, slots = conv2d_train.wgrad_plan(n, cin, cout, hw[0], hw[1], k, s)
    assert slots == 512 and tiles >= 3 * slots and tiles % slots != 0, (tiles, slots)
    assert hw[0] % 8 and hw[1] % 32
    x, w, gy, (gx64, gw64), (gxa, gwa) = _reference(shape, n, hw)
    gw = conv2d_train.conv2d_wgrad(x.to(DEV), gy.to(DEV), k, s)
    _check("gw multi-pass %s" % (shape,), gw, gw64, gwa)
    # the input gradient at the same size: 630 workgroups per image
    gx = conv2d_train.conv2d_dgrad(gy.to(DEV), w.to(DEV), s, hw[0], hw[1])
    _check("gx full size %s" % (shape,), gx, gx64, gxa)


def _layer(shape, seed):
    cin, cout, k, s = shape
    torch.manual_seed(seed)
    return torch.nn.Conv2d(cin, cout, k, stride=s, padding=k // 2, bias=False).to(DEV)


def _grads_through_run_stack(layer, x, gy):
    from mvs_amd.model import _run_stack
    xg = x.clone().requires_grad_(True)
    layer.weight.grad = None
    y = _run_stack(torch.nn.Sequential(layer), xg)
    y.backward(gy)
    return y.detach(), xg.grad, layer.weight.grad.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 16, 5, 2), (32, 32, 3, 1)], ids=_id)
def test_routing(monkeypatch, shape):
    """With "hip" tap_gemm's backward helpers raise if called and are not; with the switch unset they are called and
    gx and gw are torch.equal to _Conv2dHipTaps's."""
    from mvs_amd import tap_gemm
    cin, cout, k, s = shape
    layer = _layer(shape, 3)
    torch.manual_seed(4)
    x = torch.randn(2, cin, 21, 37, device=DEV)
    y0 = layer(x)
    gy = torch.randn_like(y0)
    calls = []

    def wrap(name):
        orig = getattr(tap_gemm._Geom, name)

        def f(self, *a, **kw):
            calls.append(name)
            return orig(self, *a, **kw)
        return f
    for name in ("scatter", "weight_grad", "to_grid", "to_par"):
        monkeypatch.setattr(tap_gemm._Geom, name, wrap(name))
    monkeypatch.delenv("MVS_TRAIN_CONV2D_BWD", raising=False)
    monkeypatch.delenv("MVS_TRAIN_CONV2D", raising=False)
    monkeypatch.delenv("MVS_TRAIN_CONV2D_FWD", raising=False)
    y_t, gx_t, gw_t = _grads_through_run_stack(layer, x, gy)
    assert "scatter" in calls and "weight_grad" in calls
    xr = x.clone().requires_grad_(True)
    layer.weight.grad = None
    tap_gemm._Conv2dHipTaps.apply(xr, layer.weight, (s, s), (k // 2, k // 2)).backward(gy)
    assert torch.equal(gx_t, xr.grad) and torch.equal(gw_t, layer.weight.grad)

    def refuse(self, *a, **kw):
        raise AssertionError("the per-tap GEMM backward was called under MVS_TRAIN_CONV2D_BWD=hip")
    for name in ("scatter", "weight_grad", "to_grid", "to_par"):
        monkeypatch.setattr(tap_gemm._Geom, name, refuse)
    monkeypatch.setenv("MVS_TRAIN_CONV2D_BWD", "hip")
    y_h, gx_h, gw_h = _grads_through_run_stack(layer, x, gy)
    assert torch.equal(y_h, y_t)                       # the same forward kernel
    assert gx_h.is_contiguous() and gx_h.shape == x.shape
    torch.testing.assert_close(gx_h, gx_t, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gw_h, gw_t, rtol=1e-4, atol=1e-3)
    # an input that needs no gradient: the input gradient is not launched (the encoder's first layer)
    from mvs_amd import conv2d_train
    seen = []
    orig_dgrad = conv2d_train.conv2d_dgrad
    monkeypatch.setattr(conv2d_train, "conv2d_dgrad", lambda *a: seen.append(1) or orig_dgrad(*a))
    layer.weight.grad = None
    conv2d_train.conv2d_hip(x, layer).backward(gy)
    assert not seen and torch.equal(layer.weight.grad, gw_h)
    conv2d_train.conv2d_hip(x.clone().requires_grad_(True), layer).backward(gy)
    assert seen
    # a gy in another layout is made contiguous by the wrapper: same bits
    layer.weight.grad = None
    xg = x.clone().requires_grad_(True)
    conv2d_train.conv2d_hip(xg, layer).backward(gy.to(memory_format=torch.channels_last))
    assert torch.equal(xg.grad, gx_h) and torch.equal(layer.weight.grad, gw_h)
    # a junk value raises where the layer would be routed
    monkeypatch.setenv("MVS_TRAIN_CONV2D_BWD", "yes")
    with pytest.raises(ValueError):
        _grads_through_run_stack(layer, x, gy)


def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


@functools.lru_cache(maxsize=None)
def _chain_reference(which):
    """The stack, its input and loss weights, and the float64 and fp32 CPU gradients (computed once)."""
    from mvs_amd import model
    spec = model._ENCODER if which == "encoder" else model._REFINE
    torch.manual_seed(11 if which == "encoder" else 12)
    seq = model._conv_bn_relu_stack(spec, torch.device("cpu")).train()
    x = torch.randn(2, spec[0][0], 36, 44)
    with torch.no_grad():
        wr = torch.randn_like(seq(x))
    grads = []
    for net, xx, ww in ((copy.deepcopy(seq).double(), x.double(), wr.double()), (copy.deepcopy(seq), x, wr)):
        xx = xx.clone().requires_grad_(True)
        (net(xx) * ww).sum().backward()
        g = {name: p.grad for name, p in net.named_parameters()}
        g["input"] = xx.grad
        grads.append(g)
    return seq, x, wr, grads[0], grads[1]


ALL_SIX = {"MVS_TRAIN_REGION_BWD": "hip", "MVS_TRAIN_S2_BWD": "hip", "MVS_TRAIN_T2_BWD": "hip",
           "MVS_TRAIN_DECONV1": "hip", "MVS_TRAIN_BN": "hip", "MVS_TRAIN_CONV2D_BWD": "hip"}


@pytest.mark.gpu
@pytest.mark.parametrize("switches", ["alone", "all_six"])
@pytest.mark.parametrize("which", ["encoder", "refine"])
def test_chain(monkeypatch, which, switches):
    """The encoder stack and the refinement stack with train-mode BatchNorm2d at 2 images of 36 x 44 through
    model._run_stack: every parameter gradient and the input gradient against float64 CPU autograd, relative L2
    <= 2 x the CPU fp32 path's own + 1e-5 (test_gpu_train.py's bound).  Every Conv2d of the stack takes both
    gradients from conv2d_train's ops (counted), none from the per-tap GEMMs (they raise)."""
    from mvs_amd import conv2d_train, tap_gemm
    from mvs_amd.model import _run_stack
    assert DEV is not None and DEV.type == "cuda" and torch.version.hip, "a HIP device is required"
    for name in tuple(ALL_SIX) + ("MVS_TRAIN_CONV2D", "MVS_TRAIN_CONV2D_FWD"):
        monkeypatch.delenv(name, raising=False)
    for name, v in (ALL_SIX.items() if switches == "all_six" else [("MVS_TRAIN_CONV2D_BWD", "hip")]):
        monkeypatch.setenv(name, v)

    def refuse(self, *a, **kw):
        raise AssertionError("the per-tap GEMM backward was called under MVS_TRAIN_CONV2D_BWD=hip")
    monkeypatch.setattr(tap_gemm._Geom, "scatter", refuse)
    monkeypatch.setattr(tap_gemm._Geom, "weight_grad", refuse)
    seen = {"conv2d_wgrad": 0, "conv2d_dgrad": 0}

    def count(name):
        orig = getattr(conv2d_train, name)

        def f(*a):
            seen[name] += 1
            return orig(*a)
        return f
    for name in seen:
        monkeypatch.setattr(conv2d_train, name, count(name))
    seq, x, wr, g64, g32 = _chain_reference(which)
    net = copy.deepcopy(seq).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    assert xg.is_cuda and all(p.is_cuda for p in net.parameters())
    (_run_stack(net, xg) * wr.to(DEV)).sum().backward()
    # one weight gradient per Conv2d, and one input gradient each too: the stack's input asks for its gradient here
    convs = sum(isinstance(m, torch.nn.Conv2d) for m in net)
    assert convs == (8 if which == "encoder" else 4)
    assert seen == {"conv2d_wgrad": convs, "conv2d_dgrad": convs}, seen
    got = {name: p.grad for name, p in net.named_parameters()}
    got["input"] = xg.grad
    assert sorted(got) == sorted(g64)
    for name in sorted(g64):
        e_g, e_c = _rel(got[name].cpu(), g64[name]), _rel(g32[name], g64[name])
        print("%s %s: gpu %.3g cpu-fp32 %.3g" % (which, name, e_g, e_c))
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
