"""GPU parity of the HIP path (C ABI via mvs_amd.ops) against the oracle and the golden vectors.

Tolerances (fp32 path; north star: 1e-4 relative on the depth map):
  * cost volume / warped volume: the HIP sampling matrices are computed in fp64 while the reference
    chains fp32 matmuls + two fp32 3x3 inverses.  Measured on config 1, the REFERENCE's own fp32
    cost volume deviates from the float64 law by up to 5.8e-4 absolute / 6.1e-5 relative L2
    (tests/test_oracle.py::test_reference_fp32_noise_level pins this), so GPU vs reference may
    differ by the sum of both errors.  Tests require
        max|gpu - ref| <= 1e-3 + 1e-3 |ref|   and   ||gpu - ref||_2 / ||ref||_2 <= 1.5e-4,
    and, the sharper check, that the GPU is no further from the float64 law than the reference's
    own fp32 result is (x 1.5 + 1e-6), on the tiny golden cases and on config-1 planes.
  * soft-argmin on identical P: 1e-5 relative (same arithmetic, different summation order).
  * end-to-end depth: 1e-4 relative on every pixel whose sort mask is not decided by a near-tie
    (|P_a - P_b| < 1e-5 relative); see test_mvsnet_end_to_end.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _t(z, k):
    return torch.from_numpy(np.asarray(z[k]))


def _close(gpu, ref, atol=1e-3, rtol=1e-3, l2=1.5e-4):
    gpu = gpu.detach().double().cpu()
    ref = torch.as_tensor(ref).double()
    assert gpu.shape == ref.shape, (gpu.shape, ref.shape)
    d = (gpu - ref).abs()
    bad = d > atol + rtol * ref.abs()
    assert not bad.any(), "max|d|=%g at %s (ref %g)" % (d.max(), d.argmax(), ref.reshape(-1)[d.argmax()])
    rel = d.norm() / max(ref.norm().item(), 1e-30)
    assert rel <= l2, "relative L2 error %g" % rel


@pytest.mark.parametrize("nv", [3, 5])
def test_fused_cost_volume_matches_golden(nv):
    from mvs_amd import warp_and_assemble_cost_volume
    z = load_golden("tiny_v%d.npz" % nv)
    B, D = int(z["batch_size"]), int(z["d_num"])
    cv, d_batch_0, ref_idx_0 = warp_and_assemble_cost_volume(
        _t(z, "K"), _t(z, "R"), _t(z, "T"), _t(z, "d_min"), _t(z, "d_int"),
        _t(z, "feat").to(DEV), B, nv, d_num=D)
    torch.cuda.synchronize()
    _close(cv, z["cv"])
    assert torch.equal(d_batch_0.cpu(), _t(z, "d_batch_0"))
    assert torch.equal(ref_idx_0, _t(z, "ref_idx_0")) and ref_idx_0.device.type == "cpu"


@pytest.mark.parametrize("nv", [3, 5])
def test_homography_warping_matches_golden(nv):
    from mvs_amd import homography_warping
    z = load_golden("tiny_v%d.npz" % nv)
    B, D = int(z["batch_size"]), int(z["d_num"])
    warped, d_batch_0, ref_idx_0 = homography_warping(
        _t(z, "K"), _t(z, "R"), _t(z, "T"), _t(z, "d_min"), _t(z, "d_int"),
        _t(z, "feat").to(DEV), B, nv, d_num=D)
    _close(warped, z["warped"])
    assert torch.equal(d_batch_0.cpu(), _t(z, "d_batch_0"))


@pytest.mark.parametrize("nv", [3, 5])
def test_assemble_cost_volume_matches_golden(nv):
    from mvs_amd import assemble_cost_volume
    z = load_golden("tiny_v%d.npz" % nv)
    cv = assemble_cost_volume(_t(z, "warped").to(DEV), nv)
    _close(cv, z["cv"], atol=1e-6, rtol=1e-6, l2=1e-7)


@pytest.mark.parametrize("nv", [3, 6, 10, 12, 14])
def test_assemble_cost_volume_tiny_values_bit_exact(nv):
    """costvolume.py:12-14 on warped values down in the subnormal range (variances and means whose
    quotients by V are subnormal, including exact ties between two subnormals): the HIP variance equals
    torch CPU's (the oracle's assemble_cost_volume, IEEE division) bit for bit for odd V and for the
    even non-power-of-two V whose ties need div_views' IEEE fallback (common.h)."""
    import mvs_oracle
    from mvs_amd import assemble_cost_volume
    g = torch.Generator().manual_seed(nv)
    n = 2 * nv * 8 * 4 * 16 * 16
    k = torch.randint(0, 1 << 23, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    sub = k.view(torch.float32) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)   # subnormals
    tiny = torch.randn(n, generator=g) * 1e-20                                                # squares subnormal
    warped = torch.where(torch.rand(n, generator=g) < 0.5, sub, tiny).reshape(2 * nv, 8, 4, 16, 16)
    got = assemble_cost_volume(warped.to(DEV), nv).cpu()
    want = mvs_oracle.assemble_cost_volume(warped, nv)
    assert (want.abs() < 1.2e-38).any() and (want != 0).any()   # the case is exercised
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), int((got != want).sum())


def test_fused_no_worse_than_reference_fp32():
    """GPU vs float64 law is within the reference's own fp32 error vs float64."""
    import mvs_oracle
    from mvs_amd import warp_and_assemble_cost_volume
    for nv in (3, 5):
        z = load_golden("tiny_v%d.npz" % nv)
        B, D = int(z["batch_size"]), int(z["d_num"])
        cv64 = mvs_oracle.cost_volume_fp64(z["feat"], z["K"], z["R"], z["T"], z["d_min"], z["d_int"],
                                           B, nv, D)
        cv, _, _ = warp_and_assemble_cost_volume(_t(z, "K"), _t(z, "R"), _t(z, "T"), _t(z, "d_min"),
                                                 _t(z, "d_int"), _t(z, "feat").to(DEV), B, nv, d_num=D)
        e_gpu = np.abs(cv.cpu().double().numpy() - cv64).max()
        e_ref = np.abs(z["cv"].astype(np.float64) - cv64).max()
        assert e_gpu <= 1.5 * e_ref + 1e-6, (e_gpu, e_ref)


def test_cfg1_cost_volume_golden_samples():
    """Config 1 (B=1, V=3, C=32, 128x160, D=48): 4096 seeded voxels + checksums."""
    from cameras import features
    from mvs_amd import warp_and_assemble_cost_volume
    z = load_golden("cfg1_cv.npz")
    shape = tuple(int(s) for s in z["shape"])
    B, C, D, h, w = shape
    feat = features(B * 3, C, h, w, seed=int(z["feat_seed"])).to(DEV)
    cv, _, _ = warp_and_assemble_cost_volume(_t(z, "K"), _t(z, "R"), _t(z, "T"), _t(z, "d_min"),
                                             _t(z, "d_int"), feat, B, 3, d_num=D)
    flat = cv.reshape(-1).cpu()
    _close(flat[torch.from_numpy(z["sample_idx"])], z["sample_val"])
    tot = flat.double().sum().item()
    assert abs(tot - float(z["total"])) <= 1e-5 * abs(float(z["total"]))
    tsq = (flat.double() ** 2).sum().item()
    assert abs(tsq - float(z["total_sq"])) <= 1e-5 * abs(float(z["total_sq"]))
    assert abs(flat.max().item() - float(z["vmax"])) <= 1e-4 * abs(float(z["vmax"]))


def test_fused_matches_oracle_distinct_depths_and_views():
    """Oracle (reference op sequence) on the CPU vs the HIP path: B=3, distinct d_min/d_int; V=9
    and V=16 run the generic kernel (more views than the staged kernel's 8)."""
    import mvs_oracle
    from cameras import camera_batch, depth_range, features
    from mvs_amd import warp_and_assemble_cost_volume
    for nv in (2, 3, 4, 6, 9, 16):
        B, C, h, w, D = 3, 12, 20, 36, 7
        K, R, T = camera_batch(B, nv, h, w, first_sample=5)
        d_min, d_int = depth_range(B, d_int=30.0, distinct=True)
        feat = features(B * nv, C, h, w, seed=100 + nv)
        cv, db, ri = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feat.to(DEV), B, nv, d_num=D)
        wr, db_ref, ri_ref = mvs_oracle.homography_warping(K, R, T, d_min, d_int, feat, B, nv, D,
                                                           concat_growth=False)
        _close(cv, mvs_oracle.assemble_cost_volume(wr, nv))
        assert torch.equal(db.cpu(), db_ref) and torch.equal(ri, ri_ref)


def test_depth_shards_concatenate_to_full_volume():
    from cameras import camera_batch, depth_range, features
    from mvs_amd import warp_and_assemble_cost_volume
    B, V, C, h, w, D = 2, 3, 32, 64, 80, 24
    K, R, T = camera_batch(B, V, h, w)
    d_min, d_int = depth_range(B, d_int=4.0)
    feat = features(B * V, C, h, w, seed=9).to(DEV)
    full, _, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feat, B, V, d_num=D)
    parts = [warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feat, B, V, d_num=D,
                                           d_begin=s, d_count=6)[0] for s in range(0, D, 6)]
    assert torch.equal(torch.cat(parts, 2), full)   # same arithmetic per plane: bit-exact


def test_full_size_properties():
    """BASELINE config 2 size (B=4, V=3, C=32, 128x160, D=192): size-independent properties."""
    from cameras import camera_batch, depth_range, features
    from mvs_amd import warp_and_assemble_cost_volume
    B, V, C, h, w, D = 4, 3, 32, 128, 160, 192
    K, R, T = camera_batch(B, V, h, w)
    d_min, d_int = depth_range(B)
    feat = features(B * V, C, h, w, seed=2).to(DEV)
    cv1, _, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feat, B, V, d_num=D)
    cv2, _, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feat, B, V, d_num=D)
    assert torch.equal(cv1, cv2)                      # deterministic forward (no atomics)
    assert torch.isfinite(cv1).all() and (cv1 >= 0).all()
    # identical views -> zero variance
    same = feat[0::V].repeat_interleave(V, 0).contiguous()
    Ks, Rs, Ts = K[0::V].repeat_interleave(V, 0), R[0::V].repeat_interleave(V, 0), T[0::V].repeat_interleave(V, 0)
    cvz, _, _ = warp_and_assemble_cost_volume(Ks, Rs, Ts, d_min, d_int, same, B, V, d_num=8)
    assert cvz.abs().max().item() <= 1e-10
    # spot-check 8 planes of every sample of the big volume against the float64 law
    import mvs_oracle
    fn = feat.cpu().numpy()
    for b in range(B):
        sl = slice(b * V, (b + 1) * V)
        for k in (0, 1, 17, 63, 100, 150, 190, 191):
            ref = mvs_oracle.cost_volume_fp64(fn[sl], K[sl], R[sl], T[sl], d_min[b:b + 1],
                                              d_int[b:b + 1], 1, V, D, d_begin=k, d_count=1)
            _close(cv1[b:b + 1, :, k:k + 1], ref, atol=1e-3, rtol=1e-3, l2=1e-4)


def test_single_view_is_zero():
    from cameras import camera_batch, depth_range, features
    from mvs_amd import warp_and_assemble_cost_volume
    K, R, T = camera_batch(2, 3, 16, 20)
    d_min, d_int = depth_range(2)
    feat = features(2, 4, 16, 20, seed=5).to(DEV)
    cv, _, _ = warp_and_assemble_cost_volume(K[0::3], R[0::3], T[0::3], d_min, d_int, feat, 2, 1, d_num=5)
    assert cv.abs().max().item() == 0.0


def _oracle_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, d_begin=0, d_count=None):
    """Autograd of the oracle's reference op sequence (fp32, the reference's own numerics)."""
    import mvs_oracle
    fc = feat.clone().requires_grad_(True)
    wr, _, _ = mvs_oracle.homography_warping(K, R, T, d_min, d_int, fc, B, nv, D, concat_growth=False)
    d_count = D - d_begin if d_count is None else d_count
    mvs_oracle.assemble_cost_volume(wr, nv)[:, :, d_begin:d_begin + d_count].backward(g)
    return fc.grad


def _law_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, d_begin=0, d_count=None):
    """Autograd of the float64 law (oracle/mvs_oracle.py::cost_volume_torch64)."""
    import mvs_oracle
    f = feat.double().clone().requires_grad_(True)
    mvs_oracle.cost_volume_torch64(f, K, R, T, d_min, d_int, B, nv, D, d_begin=d_begin,
                                   d_count=d_count).backward(g.double())
    return f.grad


def _gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, **kw):
    from mvs_amd import warp_and_assemble_cost_volume
    fg = feat.to(DEV).requires_grad_(True)
    cv, _, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, fg, B, nv, d_num=D, **kw)
    cv.backward(g.to(DEV))
    return fg.grad


def _check_grad(args, d_begin=0, d_count=None):
    """The HIP gradient against the float64 law's gradient: relative L2 <= 3e-5 and no larger than
    the reference fp32 gradient's (measured at config 1: 1.5e-5 against 6.3e-5), and no element
    further from it than the reference's own fp32 gradient is (x 1.5, + 1e-5 of the largest
    element).  The reference builds its homographies in fp32 (homography.py:40-75); its sampling
    coordinates carry ~1e-3 px of error at 160 px, which moves gradient mass between neighbouring
    taps (the tent function), so the fp32 reference itself is ~1e-2 relative from the law on
    single elements at config-1 size."""
    K, R, T, d_min, d_int, feat, g, B, nv, D = args
    kw = {} if d_count is None else {"d_begin": d_begin, "d_count": d_count}
    gpu = _gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, **kw).double().cpu()
    ref = _oracle_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, d_begin, d_count).double()
    law = _law_grad(K, R, T, d_min, d_int, feat, g, B, nv, D, d_begin, d_count)
    scale = law.abs().max().item()
    e_gpu = (gpu - law).abs().max().item()
    e_ref = (ref - law).abs().max().item()
    rel = ((gpu - law).norm() / law.norm()).item()
    rel_ref = ((ref - law).norm() / law.norm()).item()
    assert rel <= 3e-5 and rel <= rel_ref, "relative L2 %g vs float64 law (reference fp32: %g)" % (rel, rel_ref)
    assert e_gpu <= 1.5 * e_ref + 1e-5 * scale, (e_gpu, e_ref, scale)


@pytest.mark.parametrize("nv", [2, 3, 5, 9])
def test_backward_matches_autograd_of_oracle(nv):
    """mvs::cost_volume_backward against torch autograd through the oracle's reference op
    sequence (grid_sample backward + variance backward), distinct depths per sample; V=9 runs the
    generic (> 8 views) kernel."""
    from cameras import camera_batch, depth_range, features
    B, C, h, w, D = 2, 6, 18, 24, 5
    K, R, T = camera_batch(B, nv, h, w)
    d_min, d_int = depth_range(B, d_int=30.0, distinct=True)
    feat = features(B * nv, C, h, w, seed=21)
    g = torch.from_numpy(np.random.default_rng(22).standard_normal((B, C, D, h, w), dtype=np.float32))
    _close(_gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D),
           _oracle_grad(K, R, T, d_min, d_int, feat, g, B, nv, D), atol=5e-4, rtol=5e-4, l2=5e-5)
    _check_grad((K, R, T, d_min, d_int, feat, g, B, nv, D))


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 32, 128, 160, 48), (2, 5, 8, 64, 80, 40), (1, 3, 7, 37, 53, 70)])
def test_backward_config_sizes(shape, det):
    """Backward at config-1 size (B=1, V=3, C=32, 128x160, D=48: 2 plane groups of 32), V=5, and a
    ragged geometry (C not a multiple of 4, tiles cut by the image border, a partial plane group)
    against the float64 law's gradient and the oracle's fp32 autograd (_check_grad), in the
    default and the deterministic (fixed-point) mode."""
    from cameras import camera_batch, depth_range, features
    B, nv, C, h, w, D = shape
    K, R, T = camera_batch(B, nv, h, w)
    d_min, d_int = depth_range(B)
    feat = features(B * nv, C, h, w, seed=sum(shape))
    g = torch.from_numpy(np.random.default_rng(7).standard_normal((B, C, D, h, w), dtype=np.float32))
    torch.use_deterministic_algorithms(det, warn_only=True)
    try:
        _check_grad((K, R, T, d_min, d_int, feat, g, B, nv, D))
    finally:
        torch.use_deterministic_algorithms(False)


def test_backward_over_budget_footprints_and_shards():
    """A zoomed-out source camera (footprints of one plane beyond the LDS budget: taps go straight
    to the global accumulators) and a depth shard (d_begin > 0)."""
    from cameras import camera_batch, depth_range, features
    B, nv, C, h, w, D = 2, 3, 8, 128, 160, 16
    K, R, T = camera_batch(B, nv, h, w)
    K[2::3, :2, :] *= 0.2
    d_min, d_int = depth_range(B, d_int=4.0)
    feat = features(B * nv, C, h, w, seed=8)
    g = torch.from_numpy(np.random.default_rng(9).standard_normal((B, C, D, h, w), dtype=np.float32))
    _check_grad((K, R, T, d_min, d_int, feat, g, B, nv, D))
    _check_grad((K, R, T, d_min, d_int, feat, g[:, :, 8:].contiguous(), B, nv, D), d_begin=8, d_count=8)


def test_backward_deterministic_mode_at_cfg2():
    """BASELINE cfg 2 (B=4, V=3, C=32, 128x160, D=192).  Under torch.use_deterministic_algorithms
    the backward runs in 64-bit fixed point (MVS_BWD_DETERMINISTIC): two runs are bit-identical;
    the default mode (fp64 on-chip partial sums, fp32 global atomics) agrees with it to fp32
    rounding, and the gradient of sum(cv * g) is linear in g."""
    from cameras import camera_batch, depth_range, features
    B, nv, C, h, w, D = 4, 3, 32, 128, 160, 192
    K, R, T = camera_batch(B, nv, h, w)
    d_min, d_int = depth_range(B)
    feat = features(B * nv, C, h, w, seed=12)
    g = torch.randn(B, C, D, h, w, generator=torch.Generator().manual_seed(13)).to(DEV)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        a = _gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D)
        b = _gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(a, b)
    assert torch.isfinite(a).all() and a.abs().max() > 0
    f = _gpu_grad(K, R, T, d_min, d_int, feat, g, B, nv, D)
    torch.testing.assert_close(f, a, rtol=1e-5, atol=1e-5 * a.abs().max().item())
    c = _gpu_grad(K, R, T, d_min, d_int, feat, 2.0 * g, B, nv, D)
    torch.testing.assert_close(c, 2.0 * f, rtol=1e-5, atol=1e-5 * a.abs().max().item())


def test_soft_argmin_matches_golden():
    from mvs_amd import extract_depth_map
    z = load_golden("softargmin.npz")
    for key in ("ex", "rnd", "tie", "d5"):
        dep = extract_depth_map(_t(z, key + "_p").to(DEV), _t(z, key + "_d").to(DEV))
        ref = z[key + "_depth"]
        np.testing.assert_allclose(dep.cpu().numpy(), ref, rtol=1e-5, atol=0)


def test_soft_argmin_matches_oracle_random():
    """Random P vs the oracle (torch.sort as the reference calls it).  Exact ties: torch's CPU sort
    is stable only for D <= 16 (insertion sort) and implementation-defined above (introsort), so
    for D > 16 the all-tied column is checked against stable (ascending-index) semantics, which is
    what the HIP kernel implements and what the reference's own D <= 16 fixture shows."""
    import mvs_oracle
    from mvs_amd import extract_depth_map
    g = torch.Generator().manual_seed(3)
    for D in (5, 6, 16, 48, 192):
        p = torch.softmax(3 * torch.randn(2, 1, D, 17, 19, generator=g), dim=2)
        p[0, 0, :, 0, 0] = 1.0 / D      # an all-tied column
        db = (425.0 + 25.0 * torch.arange(float(D))).reshape(1, D, 1, 1).repeat(2, 1, 1, 1)
        db[1] += 50.0
        ref = mvs_oracle.extract_depth_map(p, db)
        dep = extract_depth_map(p.to(DEV), db.to(DEV)).cpu()
        if D > 16:
            n = min(5, D)
            ref[0, 0, 0, 0] = db[0, :n, 0, 0].mean()     # stable: planes 0..4 kept
        np.testing.assert_allclose(dep.numpy(), ref.numpy(), rtol=1e-5, atol=0)


def test_product_path_loads_in_tree_library():
    from mvs_amd import _lib
    import re
    lib = _lib.load()
    maps = open("/proc/self/maps").read()
    assert _lib.LIB_PATH in maps, "HIP library not mapped from the repo tree"
    assert lib.mvs_abi_version() == _lib.ABI_VERSION
    assert re.search(r"libamdhip64", maps)


def _kept_planes(P, n_est):
    """[D,h,w] -> boolean mask of the planes depthmap.py keeps (stable descending ranks)."""
    D = P.shape[0]
    t = torch.from_numpy(np.ascontiguousarray(P))
    _, order = torch.sort(t, dim=0, descending=True, stable=True)
    return (order < n_est).numpy()


@pytest.mark.parametrize("mode,arithmetic", [("eval", "fp32"), ("train", "fp32"), ("eval", "split_f16")])
def test_mvsnet_end_to_end(mode, arithmetic):
    """MVSNet.forward at config 1 (640x512, D=48): BN eval mode and the test.py:61
    train-mode-under-no_grad mode, in the default fp32 arithmetic (and eval mode in the opt-in
    split-fp16 one), against the oracle forward run on this box's CPU (the oracle
    forward is itself pinned to the reference's golden depth maps in test_oracle.py).

      * probability volumes agree to 2e-3 relative (the regulariser amplifies the reference's own
        ~1e-4 fp32 cost-volume noise; 6e-4 measured in train mode);
      * the depth map agrees to 1e-4 relative on >= 99.95 % of the pixels whose permutation mask
        (depthmap.py:11-15) is the same under both probability volumes, and to 1e-2 on all;
      * pixels whose mask flips (a near-tie of P decided differently by fp32 noise) are < 2 %
        in eval mode (train-mode BN gives flat P, where flips are common between any two
        fp32 implementations -- the CPU-vs-CPU comparison shows the same);
      * refined depth (eval): 1e-4 relative outside the 9x9 receptive field of every pixel whose
        initial depth differs (train: median 2e-4 / p99 5e-3 there -- BN batch statistics couple
        every pixel).
    """
    import mvs_oracle
    from weights import deterministic_state_dict
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    from mvs_amd import warp_and_assemble_cost_volume, extract_depth_map
    z = load_golden("cfg1_e2e.npz")
    D = int(z["d_num"])
    net = MVSNet(MVSConfig(d_num=D, arithmetic=arithmetic), device=torch.device("cpu"))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net.train() if mode == "train" else net.eval()
    img = torch.from_numpy(np.random.default_rng(int(z["img_seed"])).standard_normal(
        (3, 3, 512, 640), dtype=np.float32))
    K, R, T, d_min, d_int = (_t(z, k) for k in ("K", "R", "T", "d_min", "d_int"))
    with torch.no_grad():
        c_ini, c_ref, c_prob = mvs_oracle.mvsnet_forward(net, img, K, R, T, d_min, d_int, 1, 3, D,
                                                         (128, 160))
        if mode == "eval":
            # the box's CPU (different ISA / oneDNN kernels) is itself one more fp32 reduction
            # order: the golden depth (generated in the survey container) matches except for
            # near-tie mask flips.  In train mode (BN batch statistics, flat P) such flips are
            # frequent between any two machines, so only the same-box comparison below is made.
            same = np.abs(c_ini.numpy() - z["eval_initial"]) <= 1e-4 * np.abs(z["eval_initial"])
            assert same.mean() >= 0.98, same.mean()
        net = net.to(DEV)
        g_img = img.to(DEV)
        g_ini_full, g_ref = net(g_img, K, R, T, d_min, d_int, 1, 3)
        feats = net.feature_encoder(g_img)
        # the benchmarked feed: the fp32 channel-quad volume, or the split volume in split-fp16 arithmetic
        cv, d_batch, _ = warp_and_assemble_cost_volume(K, R, T, d_min, d_int, feats, 1, 3, d_num=D,
                                                       channel_quads=True, split=arithmetic == "split_f16")
        g_prob = net.cost_volume_reg(cv)
        g_ini = extract_depth_map(g_prob, d_batch)
    if mode == "eval":
        assert torch.equal(g_ini, g_ini_full)
    Pg = g_prob.cpu().numpy()[0, 0]
    Pc = c_prob.numpy()[0, 0]
    np.testing.assert_allclose(Pg, Pc, rtol=2e-3, atol=1e-7)
    flip = (_kept_planes(Pg, 5) != _kept_planes(Pc, 5)).any(0)
    if mode == "eval":
        assert flip.mean() < 0.02, "%.2f %% of pixels change their mask" % (100 * flip.mean())
    gi, ci = g_ini_full.cpu().numpy()[0, 0], c_ini.numpy()[0, 0]
    rel = np.abs(gi - ci) / np.abs(ci)
    bad = (rel > 1e-4) & ~flip
    # 1e-4 relative on the depth map (north star) on >= 99.95 % of unflipped pixels; the rest are
    # pixels where P's fp32 noise (<= 2e-3) reaches the depth through a small mask denominator
    assert bad.mean() <= 5e-4, "%d unflipped pixels differ; first %s" % (bad.sum(), np.argwhere(bad)[:3])
    assert rel[~flip].max() <= 1e-2, rel[~flip].max()
    # the refinement net is a 9x9-receptive-field function of the initial depth (and the image):
    # its differences must be explained by initial-depth differences inside that field
    diff = (rel > 1e-5) | flip
    halo = np.zeros_like(flip)
    for y, x in np.argwhere(diff):
        halo[max(0, y - 4):y + 5, max(0, x - 4):x + 5] = True
    gr, cr = g_ref.cpu().numpy()[0, 0], c_ref.numpy()[0, 0]
    # random-weight refinement can put a few refined depths near 0 mm: relative error against
    # max(|depth|, 100 mm) so those pixels do not divide by ~0
    rel_r = np.abs(gr - cr) / np.maximum(np.abs(cr), 100.0)
    if mode == "eval":
        bad_r = (rel_r > 1e-4) & ~halo
        assert not bad_r.any(), "refined depth differs outside halos at %d pixels" % bad_r.sum()
    else:
        # train-mode BatchNorm in the refinement net normalises with statistics of the WHOLE map,
        # so every initial-depth difference moves every refined pixel slightly
        out = rel_r[~halo]
        assert np.median(out) <= 2e-4 and np.percentile(out, 99) <= 5e-3, (
            np.median(out), np.percentile(out, 99))


@pytest.mark.parametrize("arithmetic", ["fp32", "split_f16"])
def test_pipelined_forward_is_bit_identical(arithmetic):
    """MVSNet's sample-pipelined eval forward (chunks of samples on their own streams, pipeline_chunks 2
    and 3 of B = 5) returns the one-stream forward's depth maps bit for bit: every eval kernel computes
    each sample independently.  Also the first call after a weight change (the derived-weight caches are
    formed on one lane and read on the others).  With per-sample depth ranges (d_min / d_int differing:
    the homography.py:24-26 i mod B plane tiling then depends on the whole batch) it does not pipeline."""
    from cameras import camera_batch, depth_range
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    B, V, D, H, W = 5, 3, 32, 256, 320
    torch.manual_seed(1)
    net = MVSNet(MVSConfig(d_num=D, in_h=H, in_w=W, arithmetic=arithmetic)).to(DEV).eval()
    K, R, T = camera_batch(B, V, H // 4, W // 4)
    d_min, d_int = depth_range(B, d_int=2.5)
    img = torch.randn(B * V, 3, H, W, generator=torch.Generator().manual_seed(9)).to(DEV)
    K, R, T, d_min, d_int = (t.to(DEV) for t in (K, R, T, d_min, d_int))
    import mvs_amd.model as model_mod
    lanes = []
    orig = model_mod.MVSNet._forward_one

    def spy(self, *a):
        lanes.append(model_mod._LANE[0])
        return orig(self, *a)
    with torch.no_grad():
        net.pipeline_chunks = 1
        ref = net(img, K, R, T, d_min, d_int, B, V)
        model_mod.MVSNet._forward_one = spy
        try:
            for chunks in (2, 3):
                net.pipeline_chunks = chunks
                for p in net.cost_volume_reg.conv_1_1.parameters():
                    p.mul_(1.0)   # a version bump: the derived weights are formed again, on a lane
                lanes.clear()
                got = net(img, K, R, T, d_min, d_int, B, V)
                torch.cuda.synchronize()
                assert lanes == list(range(1, chunks + 1)), lanes
                assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), chunks
            # per-sample depth ranges: one stream
            dm, di = (t.to(DEV) for t in depth_range(B, distinct=True))
            lanes.clear()
            net(img, K, R, T, dm, di, B, V)
            assert lanes == [0], lanes
        finally:
            model_mod.MVSNet._forward_one = orig


def test_rccl_world1_shard_exchange_and_interleave_at_cfg4():
    """The D-sharded path's RCCL leg on one GPU (BASELINE configs[3], SURVEY.md §8 e): an "nccl" (RCCL)
    process group of world size 1; the 8 rank slabs of cfg 4 (B = 1, V = 3, 128 x 160, D = 256, 32 planes
    each: the HIP kernel with d_begin = 32 r) go through RCCL point-to-point (batch_isend_irecv, self as
    the peer) into the owner's staging buffer [8, C, 32, h, w], and depth_shards.interleave_slabs (the
    owner-side copy exchange_to_owners runs for P > 1) forms the NCDHW volume: bit-equal to the unsharded
    D = 256 volume.  Then DepthShardedMVSNet over that group runs end to end at cfg-4 geometry and gives
    MVSNet.forward's depth maps bit for bit."""
    import socket
    import torch.distributed as dist
    from cameras import camera_batch, depth_range
    from mvs_amd import ops
    from mvs_amd.config import MVSConfig
    from mvs_amd.depth_shards import DepthShardedMVSNet, interleave_slabs
    from mvs_amd.model import MVSNet
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=DEV)
    try:
        B, V, C, H, W, D, P = 1, 3, 32, 512, 640, 256, 8
        h, w = H // 4, W // 4
        K, R, T = camera_batch(B, V, h, w)
        d_min, d_int = depth_range(B)
        feat = torch.randn(B * V, C, h, w, generator=torch.Generator().manual_seed(4)).to(DEV)
        with torch.no_grad():
            full, _ = ops.cost_volume(feat, K, R, T, d_min, d_int, B, V, 0, D, 25.0)
            slabs = [ops.cost_volume(feat, K, R, T, d_min, d_int, B, V, r * (D // P), D // P, 25.0)[0]
                     for r in range(P)]
            stage = torch.empty((P, C, D // P, h, w), device=DEV)
            reqs = dist.batch_isend_irecv([op for r in range(P) for op in (
                dist.P2POp(dist.isend, slabs[r][0].contiguous(), 0), dist.P2POp(dist.irecv, stage[r], 0))])
            for req in reqs:
                req.wait()
            out = torch.empty((C, D, h, w), device=DEV)
            interleave_slabs(stage, out)
            torch.cuda.synchronize()
        assert torch.equal(out, full[0])
        # the model end to end through the wrapper (world 1 over the RCCL group)
        net = MVSNet(MVSConfig(d_num=D, in_h=H, in_w=W)).to(DEV).eval()
        img = torch.randn(B * V, 3, H, W, generator=torch.Generator().manual_seed(8)).to(DEV)
        with torch.no_grad():
            ini_s, ref_s = DepthShardedMVSNet(net, 1, 0, group=dist.group.WORLD)(img, K, R, T, d_min, d_int, B, V)
            ini, ref = net(img, K, R, T, d_min, d_int, B, V)
        assert torch.equal(ini_s, ini) and torch.equal(ref_s, ref)
    finally:
        dist.destroy_process_group()


def test_depth_sharded_single_rank_equals_model():
    """mvs_amd.depth_shards at world size 1 (one GPU here; N > 1 is covered by the gloo test and
    the driver's multi-GPU bench) reproduces MVSNet.forward bit for bit (exact-fp32 conv_0_0 on both:
    the owner's regulariser reads the assembled NCDHW volume, which carries no bound words)."""
    from weights import deterministic_state_dict
    from cameras import camera_batch, depth_range
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    from mvs_amd.depth_shards import DepthShardedMVSNet
    D = 16
    net = MVSNet(MVSConfig(d_num=D, in_h=256, in_w=320))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net = net.to(DEV).eval()
    net.cost_volume_reg.split_f16 = False
    K, R, T = camera_batch(2, 3, 64, 80)
    d_min, d_int = depth_range(2, d_int=4.0)
    img = torch.from_numpy(np.random.default_rng(5).standard_normal((6, 3, 256, 320), dtype=np.float32)).to(DEV)
    with torch.no_grad():
        ini, ref = net(img, K, R, T, d_min, d_int, 2, 3)
        owned, ini_s, ref_s = DepthShardedMVSNet(net, 1, 0, gather=False)(img, K, R, T, d_min, d_int, 2, 3)
        ini_g, ref_g = DepthShardedMVSNet(net, 1, 0)(img, K, R, T, d_min, d_int, 2, 3)   # gathered on rank 0
    assert owned == [0, 1]
    assert torch.equal(ini, ini_s) and torch.equal(ref, ref_s)
    assert torch.equal(ini, ini_g) and torch.equal(ref, ref_g)


def test_mvsnet_opt_in_fp32_head_matches_default(monkeypatch):
    """MVSNet.forward with the opt-in fused fp32 head (MVS_FP32_HEAD=1: ops.conv_head_fp32 then conv_1_1
    on the side stream) against the default two-kernel path: conv_1_0's 864-term sums round in another
    order (fp32 accumulation error only), so the depth maps agree to 1e-4 of the depth range."""
    from weights import deterministic_state_dict
    from cameras import camera_batch, depth_range
    from mvs_amd import ops
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    D = 16
    net = MVSNet(MVSConfig(d_num=D, in_h=256, in_w=320))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net = net.to(DEV).eval()
    K, R, T = camera_batch(2, 3, 64, 80)
    d_min, d_int = depth_range(2, d_int=4.0)
    img = torch.from_numpy(np.random.default_rng(7).standard_normal((6, 3, 256, 320), dtype=np.float32)).to(DEV)
    calls = []
    orig = ops.conv_head_fp32
    monkeypatch.setattr(ops, "conv_head_fp32", lambda *a: calls.append(1) or orig(*a))
    with torch.no_grad():
        ini, ref = net(img, K, R, T, d_min, d_int, 2, 3)
        assert not calls
        monkeypatch.setenv("MVS_FP32_HEAD", "1")
        ini_h, ref_h = net(img, K, R, T, d_min, d_int, 2, 3)
    assert calls
    span = D * 4.0
    assert (ini_h - ini).abs().max().item() <= 1e-4 * span
    assert (ref_h - ref).abs().max().item() <= 1e-4 * span


@pytest.mark.parametrize("shape,wino", [((2, 32, 8, 12, 20, 40), False), ((1, 8, 1, 5, 9, 33), False),
                                        ((1, 32, 8, 7, 8, 32), False), ((2, 8, 1, 16, 24, 70), False),
                                        ((2, 32, 8, 12, 20, 40), True), ((1, 32, 8, 7, 8, 32), True),
                                        ((1, 8, 8, 9, 17, 45), True)])
def test_narrow_conv3d_matches_torch(shape, wino):
    """mvs::conv3d_k3 (csrc/conv3d_narrow.hip, CostVolumeReg.conv_0_0 / conv_out) against the torch
    fp32 Conv3d on the same device, and against float64 on the CPU: ragged x/y tiles, D not a
    multiple of the 4-depth groups, both channel counts, the direct and the depth-Winograd F(2,3)
    (wino_z, conv_0_0's inference form) sums."""
    from mvs_amd.ops import conv3d_k3
    b, cin, cout, d, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(b, cin, d, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
    ref64 = torch.nn.functional.conv3d(x.double(), wt.double(), padding=1)
    with torch.no_grad():
        y = conv3d_k3(x.to(DEV), wt.to(DEV), wino_z=wino).cpu()
        yt = torch.nn.functional.conv3d(x.to(DEV), wt.to(DEV), padding=1).cpu()
    scale = ref64.abs().max().item()
    err = (y.double() - ref64).abs().max().item()
    err_t = (yt.double() - ref64).abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)
    assert err <= 4 * err_t + 1e-6 * scale, (err, err_t)   # no worse than MIOpen's own fp32 sums


@pytest.mark.parametrize("shape", [(32, 32, 3, 1, 4, 128, 160), (16, 32, 5, 2, 2, 70, 90), (8, 16, 5, 2, 1, 33, 67),
                                   (4, 32, 3, 1, 2, 24, 50)])
def test_conv2d_channel_split_is_bit_identical(shape, monkeypatch):
    """The output-channel split of small conv2d grids (csrc/conv2d_narrow.hip launch2d: COUT over 2
    or 4 workgroups per tile) leaves every channel's sum unchanged: splits 1, 2, 4 bit-identical."""
    from mvs_amd.ops import conv2d
    cin, cout, k, st, n, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, cin, h, w, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, k, k, generator=g) * 0.2).to(DEV)
    p = [(torch.rand(cout, generator=g) + 0.5).to(DEV), torch.randn(cout, generator=g).to(DEV),
         torch.randn(cout, generator=g).to(DEV)]
    outs = []
    for sp in ("1", "2", "4"):
        monkeypatch.setenv("MVS_CONV2D_SPLIT", sp)
        with torch.no_grad():
            outs.append(conv2d(x, wt, st, *p).cpu())
    monkeypatch.delenv("MVS_CONV2D_SPLIT")
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


@pytest.mark.parametrize("shape", [(3, 8, 3, 1, 2, 37, 70), (8, 8, 3, 1, 1, 64, 96), (8, 16, 5, 2, 2, 33, 67),
                                   (16, 16, 3, 1, 1, 20, 31), (16, 32, 5, 2, 1, 40, 64),
                                   (32, 32, 3, 1, 2, 16, 40), (4, 32, 3, 1, 1, 24, 50), (32, 1, 3, 1, 2, 17, 33)])
@pytest.mark.parametrize("bn", [False, True])
def test_conv2d_matches_torch(shape, bn):
    """mvs::conv2d (csrc/conv2d_narrow.hip: the FeatureEncoder / refinement Conv2d layers,
    model.py:22-65,134-145) for every instantiated (c_in, c_out, k, stride), ragged tiles (sizes not
    multiples of the 32 x 8 tile, odd sizes under stride 2), with and without the fused eval
    BatchNorm2d + ReLU: against float64 on the CPU and no worse than the torch fp32 Conv2d (MIOpen)
    on the same device."""
    from mvs_amd.ops import conv2d
    cin, cout, k, st, n, h, w = shape
    g = torch.Generator().manual_seed(sum(shape) + bn)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.2
    ref64 = torch.nn.functional.conv2d(x.double(), wt.double(), stride=st, padding=k // 2)
    p = None
    if bn:
        p = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), torch.randn(cout, generator=g))
        ref64 = torch.clamp((ref64 - p[2].double()[:, None, None]) * p[0].double()[:, None, None]
                            + p[1].double()[:, None, None], min=0.0)
    with torch.no_grad():
        y = conv2d(x.to(DEV), wt.to(DEV), st, *([t.to(DEV) for t in p] if bn else [])).cpu()
        yt = torch.nn.functional.conv2d(x.to(DEV), wt.to(DEV), stride=st, padding=k // 2)
        if bn:
            sc, sh, mu = (t.to(DEV)[:, None, None] for t in p)
            yt = torch.clamp((yt - mu) * sc + sh, min=0.0)
        yt = yt.cpu()
    assert y.shape == ref64.shape
    scale = ref64.abs().max().item()
    err = (y.double() - ref64).abs().max().item()
    err_t = (yt.double() - ref64).abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)
    assert err <= 4 * err_t + 1e-6 * scale, (err, err_t)   # no worse than MIOpen's own fp32 sums


def test_live_regulariser_gpu_matches_full_volume():
    """Eval-mode CostVolumeReg on the GPU: live-region path (region convs + HIP conv_0_0/conv_out)
    against the full-volume MIOpen path at a cfg-1-like shape."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    D, h, w = 48, 32, 40
    pad, outpad = pad_outpad(D, h, w)
    torch.manual_seed(0)
    m = CostVolumeReg(pad=pad, outpad=outpad)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.5, 0.5)
    m = m.to(DEV).eval()
    cv = torch.rand(2, 32, D, h, w, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        live = m(cv)
        full = m.forward_full(cv)
    torch.testing.assert_close(live, full, rtol=1e-4, atol=1e-7)


def test_train_mode_live_regulariser_gpu_matches_full_volume():
    """Train-mode BN (test.py:61) on the GPU: forward_live_train (region convs + batch statistics
    from region sums and border-class constants) against forward_full, probabilities and running
    statistics, at a cfg-1-like shape."""
    import copy
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    D, h, w = 48, 32, 40
    pad, outpad = pad_outpad(D, h, w)
    torch.manual_seed(0)
    m = CostVolumeReg(pad=pad, outpad=outpad)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.5, 0.5)
    m1 = m.to(DEV).train()
    m2 = copy.deepcopy(m1)
    cv = torch.rand(2, 32, D, h, w, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        assert m1.live_train_ok(cv.shape[2:])
        live = m1(cv)
        full = m2.forward_full(cv)
    torch.testing.assert_close(live, full, rtol=1e-4, atol=1e-6)
    s1, s2 = m1.state_dict(), m2.state_dict()
    for k in s2:
        if "BN_" in k:
            torch.testing.assert_close(s1[k], s2[k], rtol=1e-5, atol=1e-6, msg=k)


def test_region_deconv_fused_epilogue_matches_torch():
    """mvs::deconv3d_k3s2 (csrc/deconv3d_region.hip): deconv_1_0 from its live input region into the
    full volume, with BN_0(eval) + ReLU + `+ y0` fused, against the torch ops on the same device
    (full-size transposed conv of the zero-extended input, then BN, ReLU, add)."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _tconv_input_region
    from mvs_amd.ops import deconv3d_k3s2
    for (D, h, w) in ((48, 32, 40), (13, 10, 17)):
        pad, outpad = pad_outpad(D, h, w)
        n = (D, h, w)
        reg = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
        g = torch.Generator().manual_seed(D)
        x_full = torch.zeros(2, 16, D, h, w)
        sl = tuple(slice(lo, hi + 1) for lo, hi in reg)
        x_full[:, :, sl[0], sl[1], sl[2]] = torch.randn(2, 16, *[hi - lo + 1 for lo, hi in reg], generator=g)
        wt = torch.randn(16, 8, 3, 3, 3, generator=g) * 0.1
        mean, var = torch.randn(8, generator=g) * 0.1, torch.rand(8, generator=g) + 0.5
        gamma, beta = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g) * 0.1
        y0 = torch.randn(2, 8, D, h, w, generator=g)
        dev = lambda t: t.to(DEV)
        with torch.no_grad():
            ref = torch.nn.functional.conv_transpose3d(dev(x_full), dev(wt), stride=2, padding=pad,
                                                       output_padding=outpad)
            ref = torch.relu((ref - dev(mean).view(1, 8, 1, 1, 1)) / torch.sqrt(dev(var) + 1e-5).view(1, 8, 1, 1, 1)
                             * dev(gamma).view(1, 8, 1, 1, 1) + dev(beta).view(1, 8, 1, 1, 1)) + dev(y0)
            x_reg = dev(x_full[:, :, sl[0], sl[1], sl[2]])
            out = deconv3d_k3s2(x_reg, [lo for lo, _ in reg], dev(wt), list(n), list(pad),
                                dev(gamma / torch.sqrt(var + 1e-5)), dev(beta), dev(mean), dev(y0))
        assert out.shape == ref.shape
        torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)


def _bn_params(c, g):
    mean, var = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1
    return gamma / torch.sqrt(var + 1e-5), beta, mean


def _bn_relu(y, sc, sh, mu):
    v = lambda t: t.view(1, -1, 1, 1, 1).to(y)
    return torch.relu((y - v(mu)) * v(sc) + v(sh))


@pytest.mark.parametrize("c,n,ncdhw,bn", [(16, (24, 20, 26), False, True), (32, (24, 20, 26), True, True),
                                         (64, (24, 20, 26), False, False), (16, (192, 128, 160), True, True),
                                         (32, (192, 128, 160), False, True), (64, (192, 128, 160), False, True)])
def test_region_s1_lds_kernel_bit_equal_to_per_lane(c, n, ncdhw, bn):
    """The fp32 path's stride-1 region convolution (conv_k_1) with and without MVS_CONV_PER_LANE: the same outputs
    bit for bit and the same bound words (written when an LDS-staged fp32 kernel, since removed as slower, ran
    without the flag; today both calls run the per-lane-operand kernel), at the live regions of a cfg-1-like and of the cfg-2 volume
    (level 1 / 2 / 3 regions: ragged 16 x 4 x TZ tiles in every dim), channels-last and channels-first."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    from mvs_amd.ops import bound_words, conv3d_region
    pad = pad_outpad(*n)[0]
    full = tuple((0, d - 1) for d in n)
    reg = _tconv_input_region(full, n, pad)
    for _ in range({16: 0, 32: 1, 64: 2}[c]):   # level 1 / 2 / 3 region (B, C2, C3)
        reg = _tconv_input_region(reg, n, pad)
    halo = _grow(reg, n, 1)
    org = lambda r: [lo for lo, _ in r]
    size = lambda r: [hi - lo + 1 for lo, hi in r]
    g = torch.Generator().manual_seed(c + n[0])
    x = torch.randn([2] + size(halo) + [c], generator=g).to(DEV)
    w27 = (torch.randn(27, c, c, generator=g) * 0.1).to(DEV)
    bnp = [t.to(DEV) for t in _bn_params(c, g)] if bn else [None] * 3
    with torch.no_grad():
        outs = []
        for per_lane in (False, True):
            yb = bound_words(1, DEV)[0]
            y = conv3d_region(x, None, w27, 0, list(n), org(reg), size(reg), org(halo), size(halo), None, *bnp,
                              out_ncdhw=ncdhw, y_bound=yb, per_lane=per_lane)
            outs.append((y, yb))
        torch.cuda.synchronize()
    (y, yb), (yp, ybp) = outs
    assert torch.equal(y, yp), (y - yp).abs().max().item()
    # the bound (the maximum over the slot words; which slot holds it depends on the wave mapping)
    bound = lambda t: float(t.cpu().numpy().view(np.float32).max())
    assert bound(yb) == bound(ybp) == y.abs().max().item()


@pytest.mark.parametrize("mode,cin,cout,ncdhw", [(1, 32, 16, False), (1, 32, 32, False), (1, 32, 64, False),
                                                 (0, 16, 16, False), (0, 32, 32, False), (0, 64, 64, False),
                                                 (2, 64, 32, False), (2, 32, 16, False), (0, 16, 16, True),
                                                 (2, 32, 16, True)])
def test_region_conv_matches_torch(mode, cin, cout, ncdhw):
    """mvs::conv3d_region (csrc/conv3d_region.hip, the regulariser's region convs on the fp32 MFMA)
    at the live regions forward_live uses (cfg-1-like volume 24 x 20 x 26 -- odd and even dims,
    both parities of P; the S2 tile is cut by the region border in every dim), channels-last and
    channels-first outputs, against torch's conv on the zero-extended tensors in float64 (CPU) and in
    fp32 on the same device: max error <= 1e-5 of the output scale and <= 4x MIOpen's own."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    from mvs_amd.ops import conv3d_region
    import torch.nn.functional as F
    n = (24, 20, 26)
    pad, outpad = pad_outpad(*n)
    full = tuple((0, d - 1) for d in n)
    Bx = _tconv_input_region(full, n, pad)
    C2 = _tconv_input_region(Bx, n, pad)
    g = torch.Generator().manual_seed(mode * 100 + cin + cout)
    sc, sh, mu = _bn_params(cout, g)
    org = lambda r: [lo for lo, _ in r]
    size = lambda r: [hi - lo + 1 for lo, hi in r]
    sl = lambda r: (slice(None), slice(None)) + tuple(slice(lo, hi + 1) for lo, hi in r)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()

    def zero_ext(reg, c):
        t = torch.zeros(2, c, *n)
        t[sl(reg)] = torch.randn(2, c, *size(reg), generator=g)
        return t

    if mode == 1:      # S2: conv_k_0 from the full cost volume onto halo(B)
        out_reg = _grow(Bx, n, 1)
        x = torch.randn(2, cin, *n, generator=g)
        wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
        f = lambda xx, ww: F.conv3d(xx, ww, stride=2, padding=pad)
        args = lambda xd: (xd, None, None, None)
        in_reg = None
    elif mode == 0:    # S1: conv_k_1 on B from halo(B)
        out_reg, in_reg = Bx, _grow(Bx, n, 1)
        x = zero_ext(in_reg, cin)
        wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
        f = lambda xx, ww: F.conv3d(xx, ww, padding=1)
    else:              # T2: deconv from C2 (+ addend) onto B
        out_reg, in_reg = Bx, C2
        x, x2 = zero_ext(in_reg, cin), zero_ext(in_reg, cin)
        wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * 0.1
        f = lambda xx, ww: F.conv_transpose3d(xx, ww, stride=2, padding=pad, output_padding=outpad)
    xin = x + x2 if mode == 2 else x
    ref64 = _bn_relu(f(xin.double(), wt.double()), sc.double(), sh.double(), mu.double())[sl(out_reg)]
    with torch.no_grad():
        reft = _bn_relu(f(xin.to(DEV), wt.to(DEV)), sc, sh, mu)[sl(out_reg)].cpu()
        conv = torch.nn.ConvTranspose3d(cin, cout, 3) if mode == 2 else torch.nn.Conv3d(cin, cout, 3)
        conv.weight.data = wt
        from mvs_amd.ops import region_weight
        w27 = region_weight(conv).to(DEV)
        if mode == 1:
            y = conv3d_region(x.to(DEV), None, w27, mode, list(n), org(out_reg), size(out_reg), None, None,
                              list(pad), sc.to(DEV), sh.to(DEV), mu.to(DEV), out_ncdhw=ncdhw)
        else:
            xr = cl(x[sl(in_reg)]).to(DEV)
            x2r = cl(x2[sl(in_reg)]).to(DEV) if mode == 2 else None
            y = conv3d_region(xr, x2r, w27, mode, list(n), org(out_reg), size(out_reg), org(in_reg),
                              size(in_reg), list(pad), sc.to(DEV), sh.to(DEV), mu.to(DEV), out_ncdhw=ncdhw)
    y = (y if ncdhw else y.permute(0, 4, 1, 2, 3)).cpu()
    assert y.shape == ref64.shape, (y.shape, ref64.shape)
    scale = ref64.abs().max().item()
    err = (y.double() - ref64).abs().max().item()
    err_t = (reft.double() - ref64).abs().max().item()
    assert err <= 1e-5 * scale, (err, scale)
    assert err <= 4 * err_t + 1e-6 * scale, (err, err_t)


def test_region_deconv_channels_last_with_addend():
    """deconv_1_0's HIP kernel reading the channels-last region sum y2 + y1 (model.py:121) equals
    its NCDHW form on the pre-added input (same arithmetic: the sum is formed on load)."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _tconv_input_region
    from mvs_amd.ops import deconv3d_k3s2
    n = (13, 10, 17)
    pad, _ = pad_outpad(*n)
    reg = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    g = torch.Generator().manual_seed(5)
    r = [hi - lo + 1 for lo, hi in reg]
    a, b = torch.randn(2, 16, *r, generator=g).to(DEV), torch.randn(2, 16, *r, generator=g).to(DEV)
    wt = (torch.randn(16, 8, 3, 3, 3, generator=g) * 0.1).to(DEV)
    sc, sh, mu = (t.to(DEV) for t in _bn_params(8, g))
    y0 = torch.randn(2, 8, *n, generator=g).to(DEV)
    with torch.no_grad():
        ref = deconv3d_k3s2(a + b, [lo for lo, _ in reg], wt, list(n), list(pad), sc, sh, mu, y0)
        got = deconv3d_k3s2(a.permute(0, 2, 3, 4, 1).contiguous(), [lo for lo, _ in reg], wt, list(n), list(pad),
                            sc, sh, mu, y0, x2=b.permute(0, 2, 3, 4, 1).contiguous(), channels_last=True)
    assert torch.equal(got, ref)


def _to_c4(x):
    """[B, C, D, H, W] -> channel-quad [B, C/4, D, H, W, 4]."""
    b, c = x.shape[:2]
    return x.reshape((b, c // 4, 4) + tuple(x.shape[2:])).permute(0, 1, 3, 4, 5, 2).contiguous()


@pytest.mark.parametrize("nv,shape", [(3, (2, 32, 24, 64, 80)), (2, (1, 8, 7, 37, 53)), (5, (1, 16, 9, 20, 36)),
                                      (8, (1, 4, 3, 16, 16))])
def test_channel_quad_cost_volume_is_the_same_values(nv, shape):
    """mvs::cost_volume_c4 (the fused kernel's 16-byte channel-quad store) holds exactly the values
    of mvs::cost_volume: bit-equal after the layout permutation, also for a depth shard."""
    from cameras import camera_batch, depth_range, features
    from mvs_amd import ops
    B, C, D, h, w = shape
    K, R, T = camera_batch(B, nv, h, w)
    d_min, d_int = depth_range(B, d_int=6.0, distinct=True)
    feat = features(B * nv, C, h, w, seed=C + D).to(DEV)
    for d_begin, d_count in ((0, D), (D // 3, D - D // 3)):
        ref, _ = ops.cost_volume(feat, K, R, T, d_min, d_int, B, nv, d_begin, d_count, 25.0)
        c4 = ops.cost_volume_c4(feat, K, R, T, d_min, d_int, B, nv, d_begin, d_count, 25.0)
        assert c4.shape == (B, C // 4, d_count, h, w, 4)
        assert torch.equal(c4, _to_c4(ref))


@pytest.mark.parametrize("shape", [(2, 32, 8, 12, 20, 40), (1, 32, 1, 7, 8, 32), (1, 8, 1, 5, 9, 33)])
def test_narrow_conv3d_channel_quad_input_is_bit_equal(shape):
    """conv3d_k3 reading the channel-quad volume sums the same products in the same order as the
    NCDHW kernel: bit-equal outputs (with and without the fused eval BN + ReLU)."""
    from mvs_amd.ops import conv3d_k3
    b, cin, cout, d, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(b, cin, d, h, w, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bn = [t.to(DEV) for t in _bn_params(cout, g)]
    with torch.no_grad():
        for p in ([None, None, None], bn):
            assert torch.equal(conv3d_k3(_to_c4(x), wt, *p, in_c4=True), conv3d_k3(x, wt, *p))


@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("shape", [(2, 24, 20, 26), (1, 48, 32, 40), (1, 8, 16, 64), (1, 7, 37, 70), (2, 12, 9, 33)])
def test_fp32_head_matches_conv0_and_float64_conv1(shape, bn):
    """ops.conv_head_fp32 (csrc/conv3d_narrow.hip C1 + the slab launches): y0 bit-equal to the
    standalone conv_0_0 kernel (conv3d_k3 in_c4 wino_z: the same VALU arithmetic), y1 = conv_1_0 +
    BN_1 + ReLU on halo(B) within fp32 accumulation error of a float64 convolution (the 864-term
    K = 27 taps x 32 channels MFMA sum: |err| <= 1e-5 * sum|x||w| |scale|), and equal to the
    per-lane stride-2 region kernel to the same tolerance.  Shapes: tile multiples (8, 16, 64: the
    windows at n - 1 come from the slab launches), odd depth, cfg-5-like odd widths, batch 2."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    from mvs_amd.ops import CONV_S2, conv3d_k3, conv3d_region, conv_head_fp32, region_weight
    b, *n = shape
    n = tuple(n)
    pad, _ = pad_outpad(*n)
    pad = [p | 1 for p in pad]   # (odd at the model's even dims; forced odd for the odd test dims)
    Bx = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    h1 = _grow(Bx, n, 1)
    o0, on = [lo for lo, _ in h1], [hi - lo + 1 for lo, hi in h1]
    g = torch.Generator().manual_seed(sum(shape) + bn)
    x = torch.randn(b, 32, *n, generator=g)
    w0 = torch.randn(8, 32, 3, 3, 3, generator=g) * 0.1
    w1 = torch.randn(16, 32, 3, 3, 3, generator=g) * 0.1
    p0 = [t.to(DEV) for t in _bn_params(8, g)] if bn else [None] * 3
    p1 = _bn_params(16, g) if bn else None
    p1d = [t.to(DEV) for t in p1] if bn else [None] * 3
    x4 = _to_c4(x.to(DEV))
    with torch.no_grad():
        y0, y1 = conv_head_fp32(x4, w0.to(DEV), *p0, w1.to(DEV), *p1d, pad, o0, on)
        torch.cuda.synchronize()
        assert torch.equal(y0, conv3d_k3(x4, w0.to(DEV), *p0, in_c4=True, wino_z=True))
        conv = torch.nn.Conv3d(32, 16, 3, bias=False)
        conv.weight.copy_(w1)
        y1r = conv3d_region(x4, None, region_weight(conv).to(DEV), CONV_S2, list(n), o0, on, None, None, pad, *p1d,
                            in_c4=True)
    sl = tuple(slice(lo, lo + k) for lo, k in zip(o0, on))
    ref = torch.nn.functional.conv3d(x.double(), w1.double(), stride=2, padding=pad)[(slice(None),) * 2 + sl]
    aref = torch.nn.functional.conv3d(x.double().abs(), w1.double().abs(), stride=2, padding=pad)[(slice(None),) * 2 + sl]
    bnmag = 0.0
    if bn:
        sc, sh, mu = [t.double().view(1, -1, 1, 1, 1) for t in p1]
        ref = torch.relu((ref - mu) * sc + sh)
        aref = aref * sc.abs()
        bnmag = ((mu * sc).abs() + sh.abs()).permute(0, 2, 3, 4, 1)   # the fp32 BN epilogue's own rounding
    ref, aref = ref.permute(0, 2, 3, 4, 1), aref.permute(0, 2, 3, 4, 1)
    tol = 1e-5 * aref + 1e-6 * bnmag + 1e-30
    for name, y in (("fused", y1), ("region kernel", y1r)):
        err = (y.double().cpu() - ref).abs()
        assert bool((err <= tol).all()), "%s: max err %.3g (tol %.3g)" % (name, err.max().item(), tol.max().item())
    assert bool(((y1 - y1r).abs().double().cpu() <= 2 * tol).all())


@pytest.mark.parametrize("c4", [True, False])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("shape", [(2, 24, 20, 26), (1, 48, 32, 40), (1, 7, 37, 70), (2, 13, 9, 33)])
def test_region_s2_lds_kernel_matches_per_lane_and_float64(shape, bn, c4):
    """conv_1_0 (S2 32 -> 16) on halo(B) through the LDS-staged kernel (csrc/conv3d_s2_lds.hip, opt-in:
    MVS_CONV_S2_LDS) against the per-lane region kernel (MVS_CONV_PER_LANE) and a float64
    convolution: both within fp32 accumulation error (|err| <= 1e-5 sum|x||w| |scale| + the BN epilogue's
    rounding), and repeatable launch to launch.  Odd extents, batch 2, channel-quad and NCDHW inputs."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    from mvs_amd.ops import CONV_S2, conv3d_region, region_weight
    b, *n = shape
    n = tuple(n)
    pad, _ = pad_outpad(*n)
    Bx = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    h1 = _grow(Bx, n, 1)
    o0, on = [lo for lo, _ in h1], [hi - lo + 1 for lo, hi in h1]
    g = torch.Generator().manual_seed(sum(shape) + 3 * bn + c4)
    x = torch.randn(b, 32, *n, generator=g)
    conv = torch.nn.Conv3d(32, 16, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(16, 32, 3, 3, 3, generator=g) * 0.1)
    p1 = _bn_params(16, g) if bn else None
    p1d = [t.to(DEV) for t in p1] if bn else [None] * 3
    xin = _to_c4(x.to(DEV)) if c4 else x.to(DEV)
    w27 = region_weight(conv).detach().to(DEV)
    args = (list(n), o0, on, None, None, list(pad), *p1d)
    with torch.no_grad():
        y = conv3d_region(xin, None, w27, CONV_S2, *args, in_c4=c4, s2_lds=True)
        y2 = conv3d_region(xin, None, w27, CONV_S2, *args, in_c4=c4, s2_lds=True)
        yp = conv3d_region(xin, None, w27, CONV_S2, *args, in_c4=c4, per_lane=True)
    assert torch.equal(y, y2)
    sl = tuple(slice(lo, lo + k) for lo, k in zip(o0, on))
    ref = torch.nn.functional.conv3d(x.double(), conv.weight.detach().double(), stride=2, padding=pad)
    aref = torch.nn.functional.conv3d(x.double().abs(), conv.weight.detach().double().abs(), stride=2, padding=pad)
    ref, aref = ref[(slice(None),) * 2 + sl], aref[(slice(None),) * 2 + sl]
    bnmag = 0.0
    if bn:
        sc, sh, mu = [t.double().view(1, -1, 1, 1, 1) for t in p1]
        ref = torch.relu((ref - mu) * sc + sh)
        aref = aref * sc.abs()
        bnmag = ((mu * sc).abs() + sh.abs()).permute(0, 2, 3, 4, 1)
    ref, aref = ref.permute(0, 2, 3, 4, 1), aref.permute(0, 2, 3, 4, 1)
    tol = 1e-5 * aref + 1e-6 * bnmag + 1e-30
    for name, got in (("lds", y), ("per-lane", yp)):
        err = (got.double().cpu() - ref).abs()
        assert bool((err <= tol).all()), "%s: max err %.3g" % (name, err.max().item())


@pytest.mark.parametrize("cout", [16, 32, 64])
def test_region_conv_s2_channel_quad_input_is_bit_equal(cout):
    """conv3d_region (CONV_S2) reading the channel-quad cost volume equals the NCDHW read bit for
    bit (the kernel feeds the MFMA the same 4 channels either way)."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    from mvs_amd.ops import CONV_S2, conv3d_region
    n = (24, 20, 26)
    pad, _ = pad_outpad(*n)
    Bx = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    out_reg = _grow(Bx, n, 1)
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(2, 32, *n, generator=g).to(DEV)
    conv = torch.nn.Conv3d(32, cout, 3)
    from mvs_amd.ops import region_weight
    w27 = region_weight(conv).detach().to(DEV)
    sc, sh, mu = [t.to(DEV) for t in _bn_params(cout, g)]
    args = (list(n), [lo for lo, _ in out_reg], [hi - lo + 1 for lo, hi in out_reg], None, None, list(pad),
            sc, sh, mu)
    with torch.no_grad():
        ref = conv3d_region(x, None, w27, CONV_S2, *args)
        y = conv3d_region(_to_c4(x), None, w27, CONV_S2, *args, in_c4=True)
    assert torch.equal(y, ref)


def test_mvsnet_channel_quad_feed_equals_ncdhw_feed():
    """MVSNet.forward's HIP inference feed (channel-quad cost volume into the live regulariser)
    against the same network fed the NCDHW volume: identical depth maps with the exact-fp32
    conv_0_0 (split_f16 off, the default fp32 arithmetic: the layouts carry the same values and sums);
    with the opt-in split-fp16 regulariser the probabilities agree to fp32 level and the depth maps to
    1e-4 outside mask flips."""
    from cameras import camera_batch, depth_range
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    import mvs_amd.costvolume as cvmod
    B, V, D, H, W = 1, 3, 32, 128, 160
    torch.manual_seed(0)
    net = MVSNet(MVSConfig(d_num=D, in_h=H, in_w=W)).to(DEV).eval()
    K, R, T = camera_batch(B, V, H // 4, W // 4)
    d_min, d_int = depth_range(B, d_int=10.0)
    img = torch.rand(B * V, 3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    calls = []
    orig = cvmod.warp_and_assemble_cost_volume
    net.cost_volume_reg.split_f16 = False

    def spy(*a, **kw):
        calls.append(kw.get("channel_quads", False))
        return orig(*a, **kw)
    import mvs_amd.model as model_mod
    with torch.no_grad():
        model_mod.warp_and_assemble_cost_volume = spy
        try:
            d4, r4 = net(img, K, R, T, d_min, d_int, B, V)
            model_mod.warp_and_assemble_cost_volume = lambda *a, **kw: orig(*a, **dict(kw, channel_quads=False))
            d5, r5 = net(img, K, R, T, d_min, d_int, B, V)
        finally:
            model_mod.warp_and_assemble_cost_volume = orig
    assert calls == [True]
    assert torch.equal(d4, d5) and torch.equal(r4, r5)
    net.cost_volume_reg.split_f16 = True
    with torch.no_grad():
        feats = net.feature_encoder(img)
        cv4, d_batch, _ = orig(K, R, T, d_min, d_int, feats, B, V, d_num=D, channel_quads=True, split=True)
        p_split = net.cost_volume_reg(cv4)
        cv, _, _ = orig(K, R, T, d_min, d_int, feats, B, V, d_num=D)
        p_exact = net.cost_volume_reg(cv)
        ds, _ = net(img, K, R, T, d_min, d_int, B, V)
    torch.testing.assert_close(p_split, p_exact, rtol=1e-4, atol=1e-9)
    flip = torch.from_numpy((_kept_planes(p_split[0, 0].cpu().numpy(), 5)
                             != _kept_planes(p_exact[0, 0].cpu().numpy(), 5)).any(0))
    rel = ((ds - d4).abs() / d4.abs())[0, 0].cpu()
    assert flip.float().mean() < 0.02 and (rel[~flip] <= 1e-4).float().mean() >= 0.9995


@pytest.mark.parametrize("channels_last,C,shape", [(True, 16, (2, 5, 7, 9)), (True, 64, (1, 6, 6, 10)),
                                                   (False, 8, (2, 6, 10, 12)), (False, 8, (1, 3, 5, 7))])
def test_channel_stats_and_bn_relu_match_torch(channels_last, C, shape):
    """csrc/channel_ops.hip (train-mode BN pieces of forward_live_train): float64 per-channel sums
    and relu(BN(x)) [+ relu(BN'(r))] against torch on the same device; channels-last and NCDHW,
    planes not a multiple of 4."""
    from mvs_amd.ops import bn_relu_, channel_stats
    g = torch.Generator().manual_seed(C + sum(shape))
    b = shape[0]
    full = (b,) + shape[1:] + (C,) if channels_last else (b, C) + shape[1:]
    x = (torch.randn(full, generator=g) * 2 + 0.5).to(DEV)
    r = torch.randn(full, generator=g).to(DEV)
    cdim = -1 if channels_last else 1
    red = [d for d in range(x.dim()) if d != cdim % x.dim()]
    s1, s2 = channel_stats(x, channels_last)
    torch.testing.assert_close(s1, x.double().sum(red), rtol=1e-12, atol=1e-9)
    torch.testing.assert_close(s2, (x.double() ** 2).sum(red), rtol=1e-12, atol=1e-9)
    p = [torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)]
    q = [torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)]
    shp = [1] * x.dim()
    shp[cdim] = C
    v = lambda t: t.view(shp)
    ref = torch.relu((x - v(p[2])) * v(p[0]) + v(p[1])) + torch.relu((r - v(q[2])) * v(q[0]) + v(q[1]))
    out = bn_relu_(x.clone(), channels_last, *p, r=r, r_bn=q)
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)
    ref1 = torch.relu((x - v(p[2])) * v(p[0]) + v(p[1]))
    torch.testing.assert_close(bn_relu_(x.clone(), channels_last, *p), ref1, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("train", [False, True])
def test_encoder_fused_bn_relu_matches_modules(train):
    """FeatureEncoder / DepthRefinement on the HIP inference path (every BatchNorm + ReLU one
    channel_ops pass; train mode: batch statistics from float64 sums and the running-statistic
    update) against the nn.Sequential itself on the same device."""
    import copy
    from mvs_amd.model import DepthRefinement, FeatureEncoder
    torch.manual_seed(0)
    for net, shape in ((FeatureEncoder(), (3, 3, 96, 128)), (DepthRefinement(), (2, 4, 40, 48))):
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.5, 1.5)
                mod.bias.data.uniform_(-0.5, 0.5)
        a = net.to(DEV).train(train)
        b = copy.deepcopy(a)
        x = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(DEV)
        with torch.no_grad():
            ya = a(x)
            yb = b.model(x) + (x[:, 0].unsqueeze(1) if isinstance(b, DepthRefinement) else 0)
        torch.testing.assert_close(ya, yb, rtol=1e-4, atol=1e-5)
        sa, sb = a.state_dict(), b.state_dict()
        for k in sb:
            torch.testing.assert_close(sa[k], sb[k], rtol=1e-5, atol=1e-6, msg=k)


@pytest.mark.parametrize("shape", [(2, 1, 48, 32, 40), (1, 1, 7, 5, 9)])
def test_softmax_depth_matches_torch(shape):
    """mvs_softmax_depth_fwd (CostVolumeReg.Norm = nn.Softmax(2), model.py:97) against torch's
    softmax on the same device."""
    from mvs_amd.ops import softmax_depth
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(shape[2])) * 4).to(DEV)
    torch.testing.assert_close(softmax_depth(x), torch.softmax(x, 2), rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("where", ["grad_cv_nan", "grad_cv_inf", "feat_inf"])
def test_backward_deterministic_mode_propagates_nonfinite(where):
    """Under torch.use_deterministic_algorithms the backward accumulates in 64-bit fixed point, which
    cannot carry NaN / Inf: a non-finite grad_cv or feature element must make the gradient NaN (as
    the default float path propagates it), never an arbitrary finite value -- NaN checks and
    GradScaler's skip logic rely on it."""
    from cameras import camera_batch, depth_range, features
    from mvs_amd import ops
    B, nv, C, h, w, D = 1, 3, 8, 24, 32, 8
    K, R, T = camera_batch(B, nv, h, w)
    d_min, d_int = depth_range(B, d_int=20.0)
    feat = features(B * nv, C, h, w, seed=4).to(DEV)
    g = torch.randn(B, C, D, h, w, generator=torch.Generator().manual_seed(5)).to(DEV)
    if where == "grad_cv_nan":
        g[0, 3, 2, 10, 11] = float("nan")
    elif where == "grad_cv_inf":
        g[0, 1, 5, 3, 4] = float("inf")
    else:
        feat[1, 2, 7, 9] = float("inf")
    _, ws = ops.cost_volume(feat, K, R, T, d_min, d_int, B, nv, 0, D, 25.0)
    det = ops.cost_volume_backward(feat, ws, g, B, nv, D, True)
    dflt = ops.cost_volume_backward(feat, ws, g, B, nv, D, False)
    assert not torch.isfinite(dflt).all()          # the float path propagates it
    assert torch.isnan(det).all()


def test_channel_stats_bit_reproducible():
    """Train-mode BN batch sums (csrc/channel_ops.hip) are slot-owned partial sums added in a fixed
    order: two runs are bit-identical (no float atomics), both layouts."""
    from mvs_amd.ops import channel_stats
    g = torch.Generator().manual_seed(11)
    for x, cl in ((torch.randn(4, 40, 33, 41, 16, generator=g), True), (torch.randn(4, 8, 48, 32, 40, generator=g), False)):
        x = x.to(DEV)
        a = channel_stats(x, cl)
        b = channel_stats(x, cl)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("distinct", [False, True])
def test_refine_glue_kernels_match_cpu_fp32(distinct):
    """ops.refine_input / refine_output (csrc/soft_argmin.hip) equal the torch sequence of
    model.py:195-205 evaluated in fp32 on the CPU (IEEE division, every op separately rounded) bit for
    bit, per-sample d_min / d_int included."""
    from cameras import depth_range
    from mvs_amd.ops import refine_input, refine_output
    B, h, w, D, scale = 3, 29, 43, 48, 1.0
    g = torch.Generator().manual_seed(12)
    d_min, d_int = depth_range(B, distinct=distinct)
    ini = d_min + D * d_int * torch.rand(B, 1, h, w, generator=g)
    img = torch.randn(B, 3, h, w, generator=g)
    conv = torch.randn(B, 1, h, w, generator=g) * 0.1
    span = d_int.mul(D).mul(scale)
    x_ref = torch.cat((torch.div(torch.subtract(ini, d_min), span), img), dim=1)
    y_ref = (conv + x_ref[:, 0].unsqueeze(1)).mul(span).add(d_min)
    with torch.no_grad():
        x = refine_input(ini.to(DEV), d_min.to(DEV), d_int.to(DEV), D, scale, img.to(DEV))
        y = refine_output(conv.to(DEV), x, d_min.to(DEV), d_int.to(DEV), D, scale)
    assert torch.equal(x.cpu(), x_ref)
    assert torch.equal(y.cpu(), y_ref)


@pytest.mark.parametrize("distinct", [False, True])
def test_refine_glue_equals_torch_sequence(distinct, monkeypatch):
    """MVSNet.refine with the two fused HIP launches equals the torch sequence on the GPU
    (MVS_REFINE_GLUE=0) bit for bit."""
    from cameras import depth_range
    from mvs_amd.config import MVSConfig
    from mvs_amd.model import MVSNet
    from weights import deterministic_state_dict
    B, V, H, W = 2, 3, 96, 128
    net = MVSNet(MVSConfig(d_num=48, in_h=H, in_w=W))
    net.load_state_dict(deterministic_state_dict(net.state_dict()))
    net = net.to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    img = torch.randn(B * V, 3, H, W, generator=g).to(DEV)
    d_min, d_int = depth_range(B, distinct=distinct)
    ini = (d_min + 48 * d_int * torch.rand(B, 1, H // 4, W // 4, generator=g)).to(DEV)
    ref_views = torch.arange(0, B * V, V)
    with torch.no_grad():
        fused = net.refine(img, ini, d_min.to(DEV), d_int.to(DEV), ref_views)
        monkeypatch.setenv("MVS_REFINE_GLUE", "0")
        ref = net.refine(img, ini, d_min.to(DEV), d_int.to(DEV), ref_views)
    assert torch.equal(fused, ref), (fused - ref).abs().max().item()


@pytest.mark.parametrize("D,scale", [(48, 1.0), (192, 2.5), (256, 0.8)])
def test_depth_hypotheses_kernel_equals_torch_expression(D, scale):
    """ops.depth_hypotheses (csrc/soft_argmin.hip) equals homography.py:24-26's expression
    d_min + d_scale * d_int * arange(D) on the CPU and on the GPU, bit for bit."""
    from cameras import depth_range
    from mvs_amd.ops import depth_hypotheses
    d_min, d_int = depth_range(3, distinct=True)
    ref = d_min + scale * d_int * torch.arange(D).reshape(1, D, 1, 1)
    gpu_expr = (d_min.to(DEV) + scale * d_int.to(DEV) * torch.arange(D, device=DEV).reshape(1, D, 1, 1)).cpu()
    with torch.no_grad():
        got = depth_hypotheses(d_min.to(DEV), d_int.to(DEV), D, scale).cpu()
    assert got.shape == ref.shape
    assert torch.equal(got, ref)
    assert torch.equal(got, gpu_expr)


@pytest.mark.parametrize("geom", [(2, 3, 8, 128, 160), (1, 5, 4, 64, 80), (1, 3, 4, 296, 400), (1, 9, 2, 32, 48)])
def test_cost_volume_bit_exact_vs_oracle_given_matrices(geom):
    """The HIP warp + variance equals the reference's fp32 arithmetic BIT FOR BIT once both sample through
    the same matrices (the ones the HIP prologue formed: fp64 algebra, stored fp32, read back from the
    op's workspace -- equal to the oracle's float64 composition up to an fp64 reordering).

    The yardstick is the exact law of tests/test_sampling_law.py (numpy, correctly rounded fp32 fma),
    which that CPU test pins bit for bit to the reference's torch CPU ops -- kornia's meshgrid,
    transform_points (torch.bmm), grid_sample, costvolume.py -- on the machine that made the golden
    fixtures.  torch's CPU kernels are not bitwise the same on every host (MKL picks its sgemm kernel
    by CPU), so the oracle's own torch result on THIS host is compared too and recorded: the share of
    differing elements and the largest difference, asserted only to stay at fp32 rounding level.
    V = 3 and 5 run the staged kernel (and the warp-only kernel), V = 9 the generic one; the
    channel-quad / split / fused-head paths are bit-equal to this output (test_cv_head.py and the
    channel-quad tests).  Widths >= 45 (every real feature width: 160, 400): torch.bmm's MKL branch.
    (Below 9 W < 400 torch multiplies the 3x3 point transform in its own loop, rounding each product
    and sum: test_sampling_law.py::test_bmm_small_width_branch.)"""
    import kornia_warp
    import mvs_oracle
    from cameras import camera_batch, depth_range
    from conftest import record_parity
    from mvs_amd import ops
    from test_sampling_law import norm_coord, sample_coord, sample_law, variance_law
    B, V, D, h, w = geom
    K, R, T = camera_batch(B, V, h, w)
    d_min, d_int = depth_range(B)
    feat = torch.randn(B * V, 32, h, w, generator=torch.Generator().manual_seed(sum(geom)))
    cv, ws = ops.cost_volume(feat.to(DEV), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
    warped_gpu = ops.homography_warp(feat.to(DEV), K, R, T, d_min, d_int, B, V, 0, D, 25.0)
    torch.cuda.synchronize()
    G = ws[:B * V * D * 9].view(B * V, D, 3, 3).cpu()
    G64 = mvs_oracle.sampling_matrices64(K, R, T, d_min, d_int, B, V, D, h, w)
    assert ((G.double() - G64).abs() <= 2 * torch.finfo(torch.float32).eps * G64.abs() + 1e-30).all()
    # the exact law
    xn, yn = norm_coord(w)[None, :], norm_coord(h)[:, None]
    fe = feat.numpy()
    law = np.empty((B * V, 32, D, h, w), np.float32)
    for i in range(B * V):
        for k in range(D):
            ix, iy = sample_coord(G[i, k].numpy().ravel(), xn, yn, h, w)
            law[i, :, k] = sample_law(fe[i], ix, iy)
    cv_law = variance_law(law.reshape(B, V, 32, D, h, w).transpose(1, 0, 2, 3, 4, 5))
    wg, cg = warped_gpu.cpu().numpy(), cv.cpu().numpy()
    # the oracle's torch ops on this host
    with torch.no_grad():
        warped = torch.stack([kornia_warp.warp_normalized(feat, G[:, k], (h, w), align_corners=False)
                              for k in range(D)], 2)
        cv_ref = mvs_oracle.assemble_cost_volume(warped, V).numpy()
    warped = warped.numpy()
    record_parity("cost_volume_bit_exact_given_matrices_%s" % "x".join(map(str, geom)),
                  warp_gpu_vs_law_differing=float((wg != law).mean()),
                  cv_gpu_vs_law_differing=float((cg != cv_law).mean()),
                  warp_gpu_vs_host_torch_differing=float((wg != warped).mean()),
                  cv_gpu_vs_host_torch_differing=float((cg != cv_ref).mean()),
                  cv_gpu_vs_host_torch_max_abs=float(np.abs(cg - cv_ref).max()))
    assert np.array_equal(wg, law), (wg != law).mean()
    assert np.array_equal(cg, cv_law), (cg != cv_law).mean()
    # torch CPU on another host (e.g. an AMD EPYC box: MKL's sgemm kernel, reduction order) rounds some
    # steps differently: fp32 rounding level relative to the volume's scale (a variance of nearly equal
    # samples cancels, so elementwise relative differences are not the measure)
    assert np.abs(cg - cv_ref).max() <= 1e-4 * np.abs(cv_ref).max(), np.abs(cg - cv_ref).max()
