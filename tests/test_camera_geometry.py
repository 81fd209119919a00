"""The cost-volume kernels at camera geometry beyond the DTU rigs (tests/synthetic_cameras.py).

Every other cost-volume test samples through the DTU scan-1 cameras, where the homogeneous
coordinate s is positive everywhere and a few percent of the samples leave the image.  The families
here run what that geometry never reaches: common.h's undivided branch (|s| <= 1e-8) and invalid
samples (NaN, infinite, far outside), sampling_matrix.h's singular inverse, the staged forward
kernel's empty, tall and over-budget footprints, cost_volume_bwd.hip's pole boxes (in LDS at
20 x 36, on global atomics at 64 x 80), its view-subset loop and its out-of-box taps, the generic
V > 8 kernels on the same inputs, and cv_head.hip's invalid-tap offset.

Forward comparisons are exact: the numpy law of tests/test_sampling_law.py, extended to non-finite
coordinates (synthetic_cameras.sample_law_ext), through the matrices the op itself formed.  The
backward is compared with a float64 reference that shares the kernel's taps
(synthetic_cameras.shared_tap_gradient) under the criterion of DESIGN.md §3.6.  Every case asserts
its family's preconditions on the CPU before it looks at a GPU result.  Measured values: DESIGN.md
§3.6a.
"""
import functools

import numpy as np
import pytest
import torch

import synthetic_cameras as sc
from synthetic_cameras import FAMILIES, SHAPES

DEV = torch.device("cuda", 0)
VIEWS = (2, 3, 5, 8, 9)      # 2..8: the staged kernels, 9: the generic ones
EPS32 = float(torch.finfo(torch.float32).eps)


def _params(V, si):
    """B, C, D of the case (V, shape index): C = 7 and 8, D = 4..6 (a partial plane group), B = 2 at
    V = 3 (two different families in the two samples)."""
    return (2 if V == 3 else 1), (7 if V in (2, 5, 9) else 8), 4 + (V + si) % 3


def _families(family, B):
    """The sample's family and, at B = 2, the next family as the second sample."""
    return (family,) if B == 1 else (family, FAMILIES[(FAMILIES.index(family) + 1) % len(FAMILIES)])


@functools.lru_cache(maxsize=4)
def _inputs(fams, V, C, D, h, w):
    K, R, T, d_min, d_int = sc.rig(fams, V, h, w)
    gen = torch.Generator().manual_seed(1000 * V + 10 * h + w + len(fams[0]))
    feat = torch.randn(len(fams) * V, C, h, w, generator=gen)
    g = torch.randn(len(fams), C, D, h, w, generator=gen)
    return K, R, T, d_min, d_int, feat, g


def _check_rigs(fams, G, V, h, w):
    """Every sample's preconditions on the matrices G [B*V, D, 3, 3]."""
    return [sc.check_preconditions(f, G[b * V:(b + 1) * V], h, w) for b, f in enumerate(fams)]


def _to_c4(cv):
    b, c, d, h, w = cv.shape
    return cv.reshape(b, c // 4, 4, d, h, w).permute(0, 1, 3, 4, 5, 2).contiguous()


# ----------------------------------------------------------------------------------------------
# CPU: the extended law and the rigs' preconditions
# ----------------------------------------------------------------------------------------------
def test_extended_law_cpu():
    """sample_law_ext is sample_law on finite coordinates, exactly 0 on non-finite ones, and torch's
    grid_sample on the pole rig wherever torch's own result is defined."""
    import kornia_warp
    from test_sampling_law import sample_law
    h, w, V, D = 37, 53, 3, 4
    assert 9 * w >= 400   # torch.bmm's MKL branch (test_sampling_law.py::test_bmm_small_width_branch)
    rng = np.random.default_rng(5)
    img = rng.standard_normal((3, h, w)).astype(np.float32)
    # finite coordinates, far outside included
    ix = np.concatenate([rng.uniform(-3, w + 2, 4000), [-1.0, -1.0000001, w, w - 1e-4, 1e30, -1e30, 3e9]]).astype(np.float32)
    iy = np.concatenate([rng.uniform(-3, h + 2, 4000), [0.5, 0.5, 0.5, h - 1e-4, 2.0, 2.0, -3e9]]).astype(np.float32)
    assert np.array_equal(sc.sample_law_ext(img, ix[None], iy[None]), sample_law(img, ix[None], iy[None]))
    bad = np.array([np.nan, np.inf, -np.inf, 1.0, np.nan], np.float32)
    ok = np.array([1.0, 1.0, np.nan, np.inf, np.nan], np.float32)
    assert (sc.sample_law_ext(img, bad[None], ok[None]) == 0).all()
    # the pole rig: s changes sign inside the image, coordinates run through +-infinity
    K, R, T, d_min, d_int = sc.rig(("pole",), V, h, w)
    G = sc.oracle_matrices64(K, R, T, d_min, d_int, 1, V, D, h, w).float()
    sc.check_preconditions("pole", G.numpy(), h, w)
    feat = torch.randn(V, 4, h, w, generator=torch.Generator().manual_seed(2))
    compared = 0
    for i in range(V):
        for k in range(D):
            want = kornia_warp.warp_normalized(feat[i:i + 1], G[i:i + 1, k], (h, w), align_corners=False)[0].numpy()
            ix, iy, _ = sc.coords(G[i, k].numpy(), h, w)
            got = sc.sample_law_ext(feat[i].numpy(), ix, iy)
            with np.errstate(invalid="ignore"):
                m = (np.abs(ix) < 1e6) & (np.abs(iy) < 1e6)
            compared += int(m.sum())
            assert np.array_equal(got[:, m], want[:, m]), (i, k, (got[:, m] != want[:, m]).mean())
    assert compared > 0.9 * V * D * h * w


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_family_preconditions_cpu(family, shape):
    """Each family's preconditions on the oracle's float64 matrices rounded to fp32 -- for the singular
    rig, which the oracle refuses (LinAlgError), on the CPU restatement of sampling_matrix.h."""
    h, w = shape
    V, D = 1 + sc.n_own_sources(family), 4
    K, R, T, d_min, d_int = sc.rig((family,), V, h, w)
    G64 = sc.oracle_matrices64(K, R, T, d_min, d_int, 1, V, D, h, w)
    assert (G64 is None) == (family == "singular")
    Ga = sc.adjugate_matrices(K, R, T, d_min, d_int, 1, V, D, h, w)
    if G64 is not None:
        G = G64.float().numpy()
        assert np.abs(Ga - G).max() <= 4 * EPS32 * np.abs(G).max()
    else:
        G = Ga
    sc.check_preconditions(family, G, h, w)


def _zoom_preconditions(K, R, T, d_min, d_int, G, D):
    from footprint import fallback_map
    h, w = sc.ZOOM_SHAPE
    fb, _ = fallback_map(K.numpy(), R.numpy(), T.numpy(), d_min.numpy(), d_int.numpy(), 1, 8, h, w, 0, D)
    assert 0.0 < fb.mean() < 1.0, fb.mean()
    rec = sc.check_preconditions("zoom", G, h, w)
    rec["fallback"] = float(fb.mean())
    return rec


def test_zoom_preconditions_cpu():
    h, w = sc.ZOOM_SHAPE
    K, R, T, d_min, d_int = sc.rig(("zoom",), 8, h, w)
    G = sc.oracle_matrices64(K, R, T, d_min, d_int, 1, 8, 8, h, w).float().numpy()
    _zoom_preconditions(K, R, T, d_min, d_int, G, 8)


# ----------------------------------------------------------------------------------------------
# a, b: forward and matrices
# ----------------------------------------------------------------------------------------------
def _matrix_ratio(G, G64):
    """Largest |G - G64| / bound over the elements; bound = 2 eps32 |G64| + 1e-30 (rounding the fp64
    result to fp32, both sides) + 64 * 2^-53 * kappa * max|G64| (fp64 roundoff amplified by the
    inverse: kappa is the 2-norm condition number of that matrix, 64 the margin for five chained
    3 x 3 products and two adjugate inverses)."""
    worst = 0.0
    for i in range(G64.shape[0]):
        for k in range(G64.shape[1]):
            m = G64[i, k].numpy()
            bound = 2 * EPS32 * np.abs(m) + 1e-30 + 64 * 2.0 ** -53 * np.linalg.cond(m, 2) * np.abs(m).max()
            worst = max(worst, float((np.abs(G[i, k].astype(np.float64) - m) / bound).max()))
    return worst


def _forward(fams, V, C, D, h, w):
    """ops.cost_volume and ops.homography_warp against the exact law through the op's own matrices.
    Returns (op matrices, oracle matrices or None, cv on the device, preconditions' records)."""
    from mvs_amd import ops
    from test_sampling_law import variance_law
    B = len(fams)
    K, R, T, d_min, d_int, feat, _ = _inputs(fams, V, C, D, h, w)
    G64 = sc.oracle_matrices64(K, R, T, d_min, d_int, B, V, D, h, w)
    if G64 is not None:
        _check_rigs(fams, G64.float().numpy(), V, h, w)
    with torch.no_grad():
        cv, ws = ops.cost_volume(feat.to(DEV), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
        warped = ops.homography_warp(feat.to(DEV), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
        torch.cuda.synchronize()
    G = ws[:B * V * D * 9].view(B * V, D, 3, 3).cpu().numpy()
    recs = _check_rigs(fams, G, V, h, w)          # the matrices that matter: the op's own
    law, _ = sc.warp_law(feat.numpy(), G, h, w)
    cv_law = variance_law(law.reshape(B, V, C, D, h, w).transpose(1, 0, 2, 3, 4, 5))
    wg, cg = warped.cpu().numpy(), cv.cpu().numpy()
    assert np.array_equal(wg, law), (fams, V, (wg != law).mean())
    assert np.array_equal(cg, cv_law), (fams, V, (cg != cv_law).mean())
    assert np.isfinite(cg).all() and (cg >= 0).all()
    return G, G64, cv, recs


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_is_the_exact_law(family, shape):
    """a, b.  Warped volume and cost volume equal the extended law bit for bit at V = 2, 3, 5, 8
    (staged kernel) and 9 (generic), the volume finite and >= 0; the op's matrices within the
    conditioned bound of the oracle's float64 ones where the oracle can form them."""
    from conftest import record_parity
    h, w = shape
    si = SHAPES.index(shape)
    worst, shares = 0.0, {}
    for V in VIEWS:
        B, C, D = _params(V, si)
        fams = _families(family, B)
        G, G64, _, recs = _forward(fams, V, C, D, h, w)
        shares = recs[0] if V == 3 else shares
        if G64 is not None:
            worst = max(worst, _matrix_ratio(G, G64))
        else:
            assert "singular" in fams
    record_parity("camera_geometry_forward_%s_%dx%d" % (family, h, w), matrix_error_over_bound=worst,
                  **{k: v for k, v in shares.items() if not isinstance(v, list)})
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_zoom_forward_and_backward():
    """The DTU rig's eight nearest views with the source intrinsics scaled by 0.2 .. 8 at 128 x 160:
    some workgroups of the staged forward kernel fit LDS and some fall back to global gathers, and
    the backward's view-subset loop splits (the largest boxes of the seven source views exceed its
    1228 slots)."""
    from conftest import record_parity
    h, w = sc.ZOOM_SHAPE
    V, C, D = 8, 8, 8
    K, R, T, d_min, d_int, feat, g = _inputs(("zoom",), V, C, D, h, w)
    G, G64, _, _ = _forward(("zoom",), V, C, D, h, w)
    rec = _zoom_preconditions(K, R, T, d_min, d_int, G, D)
    ratio = _matrix_ratio(G, G64)
    out = _backward(("zoom",), V, C, D, h, w)
    misses = out.pop("misses", [])
    record_parity("camera_geometry_zoom", matrix_error_over_bound=ratio, **rec, **out)
    assert ratio <= 1.0
    assert not misses, misses


# ----------------------------------------------------------------------------------------------
# c: the family of forward ops
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_ops_agree(family, shape):
    """c.  The channel-quad volume holds cost_volume's values, the split volume unsplits to them
    (the bound of test_bf16_cost_volume.py::test_cost_volume_family_agrees), and a depth shard with
    d_begin > 0 is the slice of the full volume (pole, behind, singular: the shard starts on the
    singular plane)."""
    from mvs_amd import ops
    h, w = shape
    B, V, C, D = 2, 3, 8, 5
    fams = _families(family, B)
    K, R, T, d_min, d_int, feat, _ = _inputs(fams, V, C, D, h, w)
    args = (feat.to(DEV), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
    with torch.no_grad():
        cv, ws = ops.cost_volume(*args)
        _check_rigs(fams, ws[:B * V * D * 9].view(B * V, D, 3, 3).cpu().numpy(), V, h, w)
        c4 = ops.cost_volume_c4(*args)
        assert torch.equal(c4, _to_c4(cv))
        scv, ams = ops.cost_volume_c4_split(*args)
        e = ops.split_exponent(ams)
        back = ops.unsplit_cost_volume(scv, ams)
        err, mag = (back - c4).abs(), c4.abs()
        upper = mag >= 2.0 ** (-3 - e)
        assert upper.any()
        assert (err[upper] <= 2.0 ** -22 * mag[upper]).all()
        assert (err[~upper] <= 2.0 ** (-25 - e)).all()
        if family in ("pole", "behind", "singular"):
            part, _ = ops.cost_volume(*args[:8], 2, 3, 25.0)
            assert torch.equal(part, cv[:, :, 2:5])
            assert torch.equal(ops.cost_volume_c4(*args[:8], 2, 3, 25.0), c4[:, :, 2:5])


@pytest.mark.gpu
@pytest.mark.parametrize("D,h,w", [(16, 29, 41), (20, 24, 40)])
@pytest.mark.parametrize("V", [2, 3])
@pytest.mark.parametrize("family", ["pole", "singular", "blind", "roll"])
def test_head_is_bit_equal_to_the_split_path(family, V, D, h, w):
    """c.  The fused head (ops.cost_volume_head) on rigs with many invalid samples: y0, y1, the
    stored box and the bound words equal the materialised split path, built as in
    test_cv_head.py::test_head_is_bit_equal_to_the_split_path."""
    from mvs_amd import ops
    from mvs_amd.config import pad_outpad
    B, C = 1, 32
    pad = list(pad_outpad(D, h, w)[0])
    assert all(p % 2 for p in pad)
    n = (D, h, w)
    h1, lo, hi = sc.regions(n, pad)
    K, R, T, d_min, d_int = sc.rig((family,), V, h, w)
    g = torch.Generator().manual_seed(D + h + w + V)
    feat = torch.randn(B * V, C, h, w, generator=g).to(DEV)
    w0 = (torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1).to(DEV)
    w1 = (torch.randn(16, 32, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bn0 = [(torch.rand(8, generator=g) + 0.5).to(DEV), (torch.randn(8, generator=g) * 0.1).to(DEV),
           (torch.randn(8, generator=g) * 0.1).to(DEV)]
    bn1 = [(torch.rand(16, generator=g) + 0.5).to(DEV), (torch.randn(16, generator=g) * 0.1).to(DEV),
           (torch.randn(16, generator=g) * 0.1).to(DEV)]
    org, size = [a for a, _ in h1], [b - a + 1 for a, b in h1]
    with torch.no_grad():
        _, ws = ops.cost_volume(feat[:, :4].contiguous(), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
        sc.check_preconditions(family, ws[:V * D * 9].view(V, D, 3, 3).cpu().numpy(), h, w)
        scv, absmax = ops.cost_volume_c4_split(feat, K, R, T, d_min, d_int, B, V, 0, D, 25.0)
        y0_ref = ops.conv3d_k3_split(scv, absmax, w0, *bn0)
        y1_ref = ops.conv_s2_split(scv, absmax, w1, list(n), org, size, pad, *bn1)
        y0, y1, box, am = ops.cost_volume_head(feat, K, R, T, d_min, d_int, B, V, 0, D, 25.0, w0, *bn0, w1, *bn1,
                                               pad, org, size, lo, hi)
        torch.cuda.synchronize()
    assert torch.equal(am, absmax)
    assert torch.equal(y0, y0_ref), (y0 - y0_ref).abs().max().item()
    assert torch.equal(y1, y1_ref), (y1 - y1_ref).abs().max().item()
    sl = (slice(None), slice(None)) + tuple(slice(a, b) for a, b in zip(lo, hi))
    assert list(box.shape) == [B, 8] + [b - a for a, b in zip(lo, hi)] + [4]
    assert torch.equal(box, scv[sl])


# ----------------------------------------------------------------------------------------------
# d: backward
# ----------------------------------------------------------------------------------------------
def _gpu_grad(fams, V, C, D, h, w, g, det):
    from mvs_amd import ops
    B = len(fams)
    K, R, T, d_min, d_int, feat, _ = _inputs(fams, V, C, D, h, w)
    torch.use_deterministic_algorithms(det, warn_only=True)
    try:
        fg = feat.to(DEV).requires_grad_(True)
        cv, ws = ops.cost_volume(fg, K, R, T, d_min, d_int, B, V, 0, D, 25.0)
        cv.backward(g.to(DEV))
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(False)
    return fg.grad.double().cpu(), ws.detach()[:B * V * D * 9].view(B * V, D, 3, 3).cpu().numpy()


def _compare_grad(gpu, ref, A, what):
    """elementwise |gpu - ref| <= 1e-5 A + 1e-9 max(A), A the scatter of the absolute
    contributions in float64 (the floor covers the fixed-point mode's resolution, about 1e-12 of the
    largest possible contribution); relative L2 <= 3e-5.  Returns (largest error / bound, largest
    |gpu - ref| / A over the elements with A >= 1e-4 max A, relative L2); the caller asserts
    error / bound <= 1 and L2 <= 3e-5 once every mode and view count has been measured and printed."""
    err = (gpu - ref).abs()
    bound = 1e-5 * A + 1e-9 * A.max()
    used = float((err / bound).max())
    big = A >= 1e-4 * A.max()
    rel_a = float((err[big] / A[big]).max())
    l2 = float((gpu - ref).norm() / ref.norm())
    print("camera geometry backward %s: error/bound %.3g, |gpu-ref|/A %.3g, L2 %.3g" % (what, used, rel_a, l2))
    return used, rel_a, l2


def _silent_views(gpu, ref, V):
    """Sample 0: view 1 (and, at V > 3, its cycled copies, which the reference finds silent too) gets
    exactly no gradient; every other view, the reference included, still gets one."""
    silent = [not ref[v].any() for v in range(V)]
    assert silent[1] and not silent[0] and silent.count(False) >= V // 2
    for v in range(V):
        assert (not gpu[v].any()) == silent[v], v


def _backward(fams, V, C, D, h, w):
    """The HIP gradient in the default and the deterministic mode against the shared-tap reference."""
    B = len(fams)
    _, _, _, _, _, feat, g = _inputs(fams, V, C, D, h, w)
    out = {}
    ref = A = None
    for det in (False, True):
        gpu, G = _gpu_grad(fams, V, C, D, h, w, g, det)
        if ref is None:
            if fams != ("zoom",):   # the zoom rig's preconditions: test_zoom_forward_and_backward
                _check_rigs(fams, G, V, h, w)
            ref, A = sc.shared_tap_gradient(feat, G, g, B, V)
        mode = "det" if det else "default"
        used, rel_a, l2 = _compare_grad(gpu, ref, A, "%s V=%d %dx%d %s" % ("+".join(fams), V, h, w, mode))
        out["bound_used_" + mode], out["err_over_A_" + mode], out["l2_" + mode] = used, rel_a, l2
        if used > 1.0 or l2 > 3e-5:
            out.setdefault("misses", []).append(("%s V=%d %s" % ("+".join(fams), V, mode), used, l2))
        if det:
            again, _ = _gpu_grad(fams, V, C, D, h, w, g, True)
            assert torch.equal(gpu, again)
        if fams[0] == "blind":
            # the blind view's own image gets no gradient; the others still do, through the mean
            _silent_views(gpu, ref, V)
    if fams[0] == "singular":
        # plane 2 alone: view 1's homography is singular there, so its image gets no gradient from
        # that plane, exactly; the other views receive theirs
        g2 = torch.zeros_like(g)
        g2[:, :, 2] = g[:, :, 2]
        gpu, G = _gpu_grad(fams, V, C, D, h, w, g2, False)
        ref2, A2 = sc.shared_tap_gradient(feat, G, g2, B, V)
        _silent_views(gpu, ref2, V)
        # one plane gives most gradient elements a single contribution, and fp32 forms 2/V g (x_v - mean)
        # to eps32 |x_v|, not eps32 |x_v - mean|: the elementwise bound in A has no sum to lean on here,
        # so this run is held to the relative L2 alone
        l2 = float((gpu - ref2).norm() / ref2.norm())
        assert l2 <= 3e-5, ("singular plane only", V, l2)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("family", FAMILIES)
def test_backward_matches_the_shared_tap_reference(family, shape):
    """d.  Autograd of ops.cost_volume at V = 2, 3, 5, 8 and 9, default and deterministic mode: the
    elementwise bound, the relative L2, two deterministic runs bit-equal; a blind view and the
    singular (view, plane) contribute exactly nothing to their own image.

    Measured on an MI355X: at most 0.037 of the elementwise bound.  With the samples
    and their mean in fp32 the kernels were at up to 0.94 (roll) and, for one of 68,635 elements of
    quarter_turn at 37 x 53 with V = 5, at 1.0375 in both modes: a sample whose x_v - mean cancels to
    0.04 .. 0.2 % of x_v on all four planes (the view shares the reference's centre, so every plane
    hits the same tap), where fp32 forms the coefficient to eps32 |x_v|.  cost_volume_bwd.hip now
    sums the samples and the mean in fp64 (sample64); that case is the regression test."""
    from conftest import record_parity
    h, w = shape
    si = SHAPES.index(shape)
    worst, misses = {}, []
    for V in VIEWS:
        B, C, D = _params(V, si)
        out = _backward(_families(family, B), V, C, D, h, w)
        misses += out.pop("misses", [])
        for k, v in out.items():
            worst[k] = max(worst.get(k, 0.0), v)
    record_parity("camera_geometry_backward_%s_%dx%d" % (family, h, w), **worst)
    assert not misses, misses   # (case, error / bound, relative L2) of every case over a bound


# ----------------------------------------------------------------------------------------------
# e: soft-argmin edges
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,n_est", [(24, 1), (24, 8), (24, 9), (24, 16), (3, 5), (3, 16)])
def test_soft_argmin_estimate_counts(D, n_est):
    """e.  extract_depth_map at the MAXE = 8 / 16 boundary (n_est = 8, 9), its ends (1, 16) and
    n_est > D (clamped), forward against the oracle and backward against float64 autograd of the
    oracle's expression.  P has no exact ties, so torch's unstable sort above 16 elements cannot
    matter and the mask is locally constant."""
    import mvs_oracle
    from mvs_amd import extract_depth_map
    gen = torch.Generator().manual_seed(100 * D + n_est)
    p = torch.softmax(3 * torch.randn(2, 1, D, 13, 19, generator=gen), dim=2)
    srt = p.sort(2).values
    assert (srt[:, :, 1:] != srt[:, :, :-1]).all()
    db = (425.0 + 25.0 * torch.arange(float(D))).reshape(1, D, 1, 1).repeat(2, 1, 1, 1)
    db[1] += 50.0
    gd = torch.randn(2, 1, 13, 19, generator=gen)
    ref = mvs_oracle.extract_depth_map(p, db, n_est)
    p64 = p.double().requires_grad_(True)
    mvs_oracle.extract_depth_map(p64, db.double(), n_est).backward(gd.double())
    pg = p.to(DEV).requires_grad_(True)
    dep = extract_depth_map(pg, db.to(DEV), n_est)
    dep.backward(gd.to(DEV))
    np.testing.assert_allclose(dep.detach().cpu().numpy(), ref.numpy(), rtol=1e-5, atol=0)
    want = p64.grad
    if n_est == 1:
        # one kept plane: depth = d_r P_r / P_r = d_r, the derivative is identically 0 and float64
        # autograd returns only its own cancellation noise (d_r / P_r - d_r P_r / P_r^2, about 1e-6
        # here); the op is held to the exact answer instead of to that noise
        assert want.abs().max() <= 1e-12 * (db.max() / p.min()).item()
        assert not pg.grad.any()
        return
    assert want.abs().max() > 0
    torch.testing.assert_close(pg.grad.cpu().double(), want, rtol=1e-5, atol=1e-5 * want.abs().max().item())
