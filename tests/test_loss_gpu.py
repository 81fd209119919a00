"""GPU: mvs_amd.loss (csrc/loss.hip) against the oracle's loss_fcn -- in float64 on the CPU for the values, its fp32
expression on the device for the gradients' bits -- and depth_accuracy against the float64 torch expression.

The bounds are derived, not measured (u = 2^-24, fp32's unit roundoff).  Every term |gt - depth| is formed and summed
in float64 by the kernel, so a per-sample sum is exact to ~2^-50; the counts are integers below 2^24, exact in fp32.
  loss_b = (float)S_b / (float)n_b      two roundings: 2 u
  loss   = sum over b of (loss0_b + loss1_b), all terms >= 0: one add per sample, B - 1 more: (B + 2) u <= (2 B + 2) u
  acc_b  = A_b / n_b                    one rounding: u;   a batch mean: B - 1 adds and one division more, (B + 1) u
           (loss_fcn's two batch means of loss_b are held to the same (B + 1) u: their worst case is one u more,
           the measured errors are at most 2 u)
  gradient: +-c or 0 with c = upstream / n_valid: loss.backward() alone gives 1 / n_valid, one fp32 division, the
            oracle's own bits; with upstream gradients on all three outputs (g_loss + g_acc / B) / n_valid is three
            roundings, 3 u < 2^-22 where the two terms have one sign (the test's upstream gradients keep the
            cancellation below 1.2x: within 2^-22 all the same).
"""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = 2.0 ** -24
# a single pixel; below one float4; ragged tails; (40, 67): three workgroups per sample in one pass
SHAPES = [(1, 1), (1, 3), (2, 3), (5, 7), (9, 33), (17, 40), (40, 67)]
CASES = [(B, h, w) for B in (1, 3) for h, w in SHAPES]


def _maps(B, h, w, seed=0):
    """gt with ~30 % exact zeros, negative depths, a valid first pixel per sample; for B > 1 sample 1 has exactly one
    valid pixel; initial == gt exactly at ~10 % of the pixels and (h * w > 1) at sample 0's last pixel, which is
    valid."""
    g = torch.Generator().manual_seed(1000 * B + 10 * h + w + seed)
    shape = (B, 1, h, w)
    gt = 300.0 + 250.0 * torch.randn(shape, generator=g)
    gt[torch.rand(shape, generator=g) < 0.3] = 0.0
    gt[:, 0, 0, 0] = torch.tensor([451.5, -37.25, 612.0][:B])
    if B > 1:
        gt[1, 0].view(-1)[1:] = 0.0
    initial = gt + 6.0 * torch.randn(shape, generator=g)
    refined = gt + 2.0 * torch.randn(shape, generator=g)
    ties = torch.rand(shape, generator=g) < 0.1
    ties[:, 0, 0, 0] = False
    if h * w > 1:
        gt[0, 0, -1, -1] = 207.125
        ties[0, 0, -1, -1] = True
    initial = torch.where(ties, gt, initial)
    return gt, initial, refined


_ORACLE = {}


def _oracle(key, gt, initial, refined):
    """(float64 CPU values, fp32 device gradients of the oracle's expression under loss.backward()), computed once."""
    if key not in _ORACLE:
        import mvs_oracle
        with torch.no_grad():
            v64 = [float(v) for v in mvs_oracle.loss_fcn(gt.double(), initial.double(), refined.double())]
        i, r = (t.to(DEV).requires_grad_(True) for t in (initial, refined))
        mvs_oracle.loss_fcn(gt.to(DEV), i, r)[0].backward()
        _ORACLE[key] = (v64, i.grad, r.grad)
    return _ORACLE[key]


def _check_values(got, v64, B, what):
    loss, a0, a1 = (float(v.detach()) for v in got)
    print("%s: loss rel err %.3g u (bound %d u), acc rel err %.3g u, %.3g u (bound %d u)"
          % (what, abs(loss - v64[0]) / v64[0] / U, 2 * B + 2, abs(a0 - v64[1]) / max(v64[1], 1e-300) / U,
             abs(a1 - v64[2]) / v64[2] / U, B + 1))
    assert abs(loss - v64[0]) <= (2 * B + 2) * U * v64[0], (what, loss, v64[0])
    assert abs(a0 - v64[1]) <= (B + 1) * U * v64[1], (what, a0, v64[1])
    assert abs(a1 - v64[2]) <= (B + 1) * U * v64[2], (what, a1, v64[2])


def _run(gt, initial, refined):
    """loss_fcn on the device and loss.backward(): (the three values, g_initial, g_refined)."""
    from mvs_amd.loss import loss_fcn
    i, r = (t.to(DEV).requires_grad_(True) for t in (initial, refined))
    gt_d = gt.to(DEV).requires_grad_(True)
    out = loss_fcn(gt_d, i, r)
    out[0].backward()
    assert gt_d.grad is None
    assert all(o.dim() == 0 and o.dtype == torch.float32 and o.device == DEV for o in out)
    return out, i.grad, r.grad


@pytest.mark.parametrize("B,h,w", CASES)
def test_forward_against_float64_and_gradient_bits(B, h, w):
    gt, initial, refined = _maps(B, h, w)
    v64, gi, gr = _oracle((B, h, w), gt, initial, refined)
    out, g0, g1 = _run(gt, initial, refined)
    _check_values(out, v64, B, "B=%d %dx%d" % (B, h, w))
    assert torch.equal(g0, gi) and torch.equal(g1, gr)
    # zero exactly at the invalid pixels and at the exact ties
    gt_d, tie = gt.to(DEV), (gt == initial).to(DEV)
    assert (g0[gt_d == 0] == 0).all() and (g1[gt_d == 0] == 0).all() and (g0[tie] == 0).all()
    assert (g1[gt_d != 0] != 0).all()
    if h * w > 1:
        assert tie[0, 0, -1, -1] and gt[0, 0, -1, -1] != 0
    # the same under no_grad, and the op's own outputs
    from mvs_amd.loss import loss_fcn, masked_mae
    with torch.no_grad():
        again = loss_fcn(gt.to(DEV), initial.to(DEV), refined.to(DEV))
        n_valid = masked_mae(gt.to(DEV), initial.to(DEV), refined.to(DEV), 0.05)[4]
    assert all(torch.equal(a, b) for a, b in zip(again, out))
    assert torch.equal(n_valid.cpu(), (gt != 0).sum((1, 2, 3)).float())
    if B > 1:
        assert n_valid[1].item() == 1.0


@pytest.mark.parametrize("B,h,w", [(1, 5, 7), (3, 9, 33), (3, 40, 67)])
def test_gradients_through_all_three_outputs(B, h, w):
    """Upstream gradients on loss, initial_acc and refined_acc at once, against float64 autograd per element."""
    import mvs_oracle
    from mvs_amd.loss import loss_fcn
    gt, initial, refined = _maps(B, h, w)
    ups = [torch.tensor(v, dtype=torch.float32) for v in (0.7, 1.3, -0.25)]
    i64, r64 = (t.double().requires_grad_(True) for t in (initial, refined))
    want = torch.autograd.grad(mvs_oracle.loss_fcn(gt.double(), i64, r64), (i64, r64), [u.double() for u in ups])
    i, r = (t.to(DEV).requires_grad_(True) for t in (initial, refined))
    got = torch.autograd.grad(loss_fcn(gt.to(DEV), i, r), (i, r), [u.to(DEV) for u in ups])
    for g, g64 in zip(got, want):
        g = g.cpu().double()
        err = ((g - g64).abs() / g64.abs().clamp_min(1e-300)).max().item()
        print("B=%d %dx%d: gradient max rel err %.3g u (bound 4 u)" % (B, h, w, err / U))
        assert ((g - g64).abs() <= 2.0 ** -22 * g64.abs()).all()
        assert (g[g64 == 0] == 0).all() and (g64 == 0).any()


def _nan_pattern_case(gt, initial, refined):
    import mvs_oracle
    from mvs_amd.loss import depth_accuracy
    i, r = (t.to(DEV).requires_grad_(True) for t in (initial, refined))
    want = mvs_oracle.loss_fcn(gt.to(DEV), i, r)
    want[0].backward()
    out, g0, g1 = _run(gt, initial, refined)
    for a, b in zip(out, want):
        assert torch.isnan(a).item() == torch.isnan(b).item()
    for g, gw in ((g0, i.grad), (g1, r.grad)):
        assert torch.equal(torch.isnan(g), torch.isnan(gw))
        assert torch.equal(torch.nan_to_num(g, nan=7.0), torch.nan_to_num(gw, nan=7.0))
    acc = depth_accuracy(gt.to(DEV), initial.to(DEV), refined.to(DEV))
    return out, g0, g1, acc


def test_sample_without_a_valid_pixel():
    from mvs_amd.loss import masked_mae
    gt, initial, refined = _maps(3, 9, 33)
    clean = _run(gt, initial, refined)
    gt[2] = 0.0
    out, g0, g1, acc = _nan_pattern_case(gt, initial, refined)
    assert all(torch.isnan(o) for o in out) and all(torch.isnan(a) for a in acc)
    assert torch.isnan(g0[2]).all() and torch.isnan(g1[2]).all()
    # the other samples' gradients are what they were
    assert torch.equal(g0[:2], clean[1][:2]) and torch.equal(g1[:2], clean[2][:2])
    with torch.no_grad():
        per = masked_mae(gt.to(DEV), initial.to(DEV), refined.to(DEV), 0.05)
    for v in per[:4]:
        assert torch.isnan(v[2]) and not torch.isnan(v[:2]).any()
    assert per[4].tolist() == [float((gt[b] != 0).sum()) for b in range(3)] and per[4][2] == 0


def test_nan_in_gt_is_valid_and_poisons_its_sample_only():
    from mvs_amd.loss import masked_mae
    gt, initial, refined = _maps(3, 9, 33)
    clean = _run(gt, initial, refined)
    with torch.no_grad():
        per_clean = masked_mae(gt.to(DEV), initial.to(DEV), refined.to(DEV), 0.05)
    was_valid = bool(gt[0, 0, 3, 5] != 0)
    gt[0, 0, 3, 5] = float("nan")
    out, g0, g1, _ = _nan_pattern_case(gt, initial, refined)
    assert all(torch.isnan(o) for o in out)
    with torch.no_grad():
        per = masked_mae(gt.to(DEV), initial.to(DEV), refined.to(DEV), 0.05)
    assert per[4][0] == per_clean[4][0] + (0.0 if was_valid else 1.0)      # counted as valid
    assert torch.isnan(per[0][0]) and torch.isnan(per[1][0])
    assert per[2][0] < 1.0 or per[4][0] == 1                                # never accurate
    for a, b in zip(per, per_clean):
        assert torch.equal(a[1:], b[1:])
    assert torch.equal(g0[1:], clean[1][1:]) and torch.equal(g1[1:], clean[2][1:])
    assert not torch.isnan(g0[1:]).any()


def _dyadic(B, h, w, thresh, seed):
    """gt multiples of 1/8 in [-64, 64] (~30 % zeros), differences multiples of 1/64: |gt - depth| and thresh * |gt|
    (a multiple of 1/128) are exact in fp32 and float64 alike.  Where gt is a non-zero integer (about one pixel in
    nine) the pixel sits exactly ON the boundary: initial = gt + thresh |gt|, refined = gt - thresh |gt|."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, 1, h, w)
    gt = torch.randint(-512, 513, shape, generator=g).float() / 8.0
    gt[torch.rand(shape, generator=g) < 0.3] = 0.0
    gt[:, 0, 0, 0] = 24.0
    gt[:, 0, 0, 1] = 2.125
    d0 = torch.randint(-160, 161, shape, generator=g).float() / 64.0
    d1 = torch.randint(-40, 41, shape, generator=g).float() / 64.0
    d0[:, 0, 0, 1] = d1[:, 0, 0, 1] = 1.0                # one pixel per sample outside both thresholds for sure
    on = (gt == gt.round()) & (gt != 0)
    initial = torch.where(on, gt + thresh * gt.abs(), gt + d0)
    refined = torch.where(on, gt - thresh * gt.abs(), gt + d1)
    return gt, initial, refined, on


@pytest.mark.parametrize("thresh", [0.25, 0.0625])
@pytest.mark.parametrize("B,h,w", [(1, 5, 7), (3, 17, 40), (3, 40, 67)])
def test_depth_accuracy_counts_on_a_dyadic_grid(B, h, w, thresh):
    from mvs_amd.loss import depth_accuracy, masked_mae
    gt, initial, refined, on = _dyadic(B, h, w, thresh, seed=B * h + w)
    g64, valid = gt.double(), gt != 0
    n64 = valid.sum((1, 2, 3))
    counts = [(valid & ((g64 - x.double()).abs() <= thresh * g64.abs())).sum((1, 2, 3)) for x in (initial, refined)]
    assert on.any() and all((c > on.sum((1, 2, 3)) - 1).all() and (c < n64).any() for c in counts)
    with torch.no_grad():
        per = [v.cpu() for v in masked_mae(gt.to(DEV), initial.to(DEV), refined.to(DEV), thresh)]
    assert torch.equal(per[4], n64.float())
    for acc, c in zip(per[2:4], counts):
        assert torch.equal(acc, c.float() / n64.float())        # the count, as its correctly rounded quotient
        assert ((acc.double() - c.double() / n64.double()).abs() <= U * c.double() / n64.double()).all()
    fracs = depth_accuracy(gt.to(DEV), initial.to(DEV), refined.to(DEV), thresh)
    for f, c in zip(fracs, counts):
        want = (c.double() / n64.double()).mean().item()
        assert f.dim() == 0 and not f.requires_grad and abs(f.item() - want) <= (B + 1) * U * want
    # every valid pixel ON the boundary is accurate; one step of 1/64 outside it none is
    edge = torch.where(valid, gt.round() + (gt == 0).float(), gt)       # integer depths where valid
    lim = thresh * edge.abs()
    f0, f1 = depth_accuracy(edge.to(DEV), (edge + lim).to(DEV), (edge - lim).to(DEV), thresh)
    assert f0.item() == 1.0 and f1.item() == 1.0
    f0, f1 = depth_accuracy(edge.to(DEV), (edge + lim + 1 / 64).to(DEV), (edge - lim - 1 / 64).to(DEV), thresh)
    assert f0.item() == 0.0 and f1.item() == 0.0


def test_results_do_not_depend_on_the_workspace():
    from mvs_amd import _lib, loss
    gt, initial, refined = (t.to(DEV) for t in _maps(3, 40, 67))
    words = _lib.load().mvs_masked_mae_workspace_bytes(3, 40, 67) // 8
    assert words == 3 * 3 * 5
    runs = []
    for fill in (float("nan"), 0.0, None):
        ws = None if fill is None else torch.full((words + 16,), fill, device=DEV, dtype=torch.float64)
        runs.append([v.view(torch.int32).clone() for v in loss._forward(gt, initial, refined, 0.05, ws)])
        if ws is not None:
            assert (torch.isnan(ws[words:]) if fill != 0.0 else ws[words:] == 0).all()    # nothing past the slots
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))
    with pytest.raises(ValueError):
        loss._forward(gt, initial, refined, 0.05, torch.zeros(words - 1, device=DEV, dtype=torch.float64))


def test_multi_pass_walk():
    """Sized from the plan: every workgroup makes 3 passes over a sample, the last one ragged, the last item of a
    sample three elements; samples 1 and 2 start off a 16-byte boundary (the scalar path), sample 0 on one."""
    from mvs_amd import loss
    B = 3
    wg, _ = loss.plan(B, 1, 2 ** 22)
    items = 2 * wg * 256 + 777
    n = 4 * items - 1
    assert loss.plan(B, 1, n) == (wg, 3) and wg > 1 and items % (wg * 256) != 0 and (n * 4) % 16 != 0
    g = torch.Generator().manual_seed(77)
    gt = 300.0 + 250.0 * torch.randn((B, 1, 1, n), generator=g)
    gt[torch.rand(gt.shape, generator=g) < 0.3] = 0.0
    initial = gt + 6.0 * torch.randn(gt.shape, generator=g)
    refined = gt + 2.0 * torch.randn(gt.shape, generator=g)
    initial[:, :, :, ::11] = gt[:, :, :, ::11]
    v64, gi, gr = _oracle("multi-pass", gt, initial, refined)
    out, g0, g1 = _run(gt, initial, refined)
    _check_values(out, v64, B, "multi-pass B=%d n=%d" % (B, n))
    assert torch.equal(g0, gi) and torch.equal(g1, gr)


def test_non_contiguous_and_misaligned_inputs():
    from mvs_amd.loss import depth_accuracy, loss_fcn
    B, h, w = 3, 9, 33
    gt, initial, refined = (t.to(DEV) for t in _maps(B, h, w))
    big = torch.randn(B, 3, h, w, device=DEV)
    big[:, 1] = initial[:, 0]
    big.requires_grad_(True)
    flat = torch.zeros(B * h * w + 5, device=DEV)
    flat[1:1 + B * h * w] = gt.reshape(-1)
    gt_off = flat[1:1 + B * h * w].view(B, 1, h, w)
    assert gt_off.data_ptr() % 16 == 4 and gt_off.is_contiguous() and not big[:, 1:2].is_contiguous()
    r_a, r_b = (refined.clone().requires_grad_(True) for _ in range(2))
    i_b = initial.clone().requires_grad_(True)
    got = loss_fcn(gt_off, big[:, 1:2], r_a)
    want = loss_fcn(gt.clone(), i_b, r_b)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    got[0].backward()
    want[0].backward()
    assert torch.equal(big.grad[:, 1:2], i_b.grad) and torch.equal(r_a.grad, r_b.grad)
    assert (big.grad[:, 0] == 0).all() and (big.grad[:, 2] == 0).all()
    for a, b in zip(depth_accuracy(gt_off, big[:, 1:2], r_a, 0.02), depth_accuracy(gt.clone(), i_b, r_b, 0.02)):
        assert torch.equal(a, b)


def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


def test_train_step_with_the_package_loss():
    """tests/test_gpu_train.py's cfg-1 step with mvs_amd.loss.loss_fcn in the oracle's place, against the same
    fixture (tests/golden/train_step_cfg1.npz: the float64-law gradients and the fp32 CPU run's distance to them):
    every parameter's gradient within 2x the CPU fp32 gradient's distance + 1e-5."""
    from conftest import load_golden
    from make_train_step import GEOM, train_step_inputs
    from mvs_amd.loss import loss_fcn
    B, V, D, H, W = GEOM
    gold = load_golden("train_step_cfg1.npz")
    net, img, K, R, T, d_min, d_int, gt = train_step_inputs()
    net_g = copy.deepcopy(net).to(DEV)
    ini_g, ref_g = net_g(img.to(DEV), K, R, T, d_min, d_int, B, V)
    loss_g, acc1_g, acc2_g = loss_fcn(gt.to(DEV), ini_g, ref_g)
    loss_g.backward()
    torch.cuda.synchronize()
    lg, lc, ld = loss_g.item(), float(gold["loss_cpu_fp32"]), float(gold["loss_f64"])
    pg = dict(net_g.named_parameters())
    names = sorted(k[4:] for k in gold.files if k.startswith("g64/"))
    assert set(pg) == set(names) and len(pg) > 0
    assert all(pg[n].grad is not None for n in names)
    worst = {n: (_rel(pg[n].grad.cpu(), torch.from_numpy(gold["g64/" + n])), float(gold["ec/" + n])) for n in names}
    print("train step, package loss: loss %.9g (cpu fp32 %.9g, float64 %.9g); worst gradient ratio %.3g"
          % (lg, lc, ld, max(a / (2.0 * b + 1e-5) for a, b in worst.values())))
    assert np.isfinite(lg) and np.isfinite(acc1_g.item()) and np.isfinite(acc2_g.item())
    assert abs(lg - ld) <= 3 * abs(lc - ld) + 1e-4 * abs(ld), (lg, lc, ld)      # (that test's bound on the loss)
    for name, (e_g, e_c) in worst.items():
        assert torch.isfinite(pg[name].grad).all(), name
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
