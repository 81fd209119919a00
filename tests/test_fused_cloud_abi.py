"""CPU: the fused point cloud (include/fusion/mvs_view_fusion.h, mvs_amd.fusion.fused_point_cloud) -- header, exports
and bindings in sync, the workspace query, every refusal before any launch (dimensions and fake pointers only: no
memory is touched), the op's schema and fake kernel, the host-side argument checks, and the float64 restatement's own
conditions on the plane scenes the GPU tests use.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import fused_cloud_ref
import fusion_cases
from conftest import REPO

HEADER = os.path.join(REPO, "include", "fusion", "mvs_view_fusion.h")
NAMES = ("mvs_fuse_views_workspace_bytes", "mvs_fuse_views_fwd")
NULL, FAKE, ODD = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001)
C_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
INF, NAN = float("inf"), float("nan")
# (emitted, kept) per scene, from the numpy prototype the rule was written with
EMITTED_KEPT = {(128, 160, 5, 4): (22869, 81916), (17, 40, 5, 10): (742, 3289), (9, 33, 5, 4): (322, 1166),
                (5, 7, 5, 10): (44, 155), (128, 160, 2, 1): (20482, 40039)}


def _header_signatures():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^\s*(int|size_t)\s+(mvs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        types = [ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]] for a in args.split(",")]
        out[name] = (C_TYPES[res], types)
    return out


def test_header_exports_and_bindings():
    from mvs_amd import _build, _lib, fusion
    lib = _lib.load()
    declared = _header_signatures()
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.FUSE_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        for table in (_lib.SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.LOSS_SIGNATURES, _lib.FILTER_SIGNATURES):
            assert name not in table
        res, args = _lib.FUSE_SIGNATURES[name]
        assert (res, list(args)) == declared[name], name
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 24                   # additive: not bumped
    assert HEADER in [os.path.abspath(p) for p in _build.HEADERS]
    assert any(os.path.basename(p) == "depth_fuse.hip" for p in _build.SOURCES)
    assert "depth_fuse.hip" not in _build.SOURCE_FLAGS                       # default build flags
    assert callable(fusion.fused_point_cloud) and hasattr(torch.ops.mvs_fusion, "fuse_views")
    assert not hasattr(torch.ops.mvs, "fuse_views")
    assert "fused_point_cloud" in fusion.point_cloud.__doc__ and "fused_point_cloud" in fusion.__doc__


def test_workspace_bytes():
    from mvs_amd import _lib
    lib = _lib.load()
    for n, h, w in ((1, 1, 1), (2, 2, 2), (5, 17, 40), (49, 128, 160), (5, 296, 400)):
        assert lib.mvs_fuse_views_workspace_bytes(n, h, w) == n * h * w
    for n, h, w in ((0, 4, 4), (-1, 4, 4), (5, 0, 4), (5, 4, -2), (2, 32768, 32768), (1, 2 ** 31 - 1, 2),
                    (2 ** 20, 64, 32)):
        assert lib.mvs_fuse_views_workspace_bytes(n, h, w) == 0, (n, h, w)


def test_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()
    names = ("depth", "mask", "colors", "K", "R", "T", "pairs", "mat", "used", "emitted", "merged", "xyz", "rgb")

    def fuse(n=5, s=4, h=5, w=7, px=1.0, rel=0.01, **kw):
        p = {k: kw.pop(k, FAKE) for k in names}
        assert not kw
        return lib.mvs_fuse_views_fwd(p["depth"], p["mask"], p["colors"], p["K"], p["R"], p["T"], p["pairs"], p["mat"],
                                      n, s, h, w, px, rel, p["used"], p["emitted"], p["merged"], p["xyz"], p["rgb"],
                                      NULL)

    # pointers: non-null (colors and rgb: both or neither); floats and ints 4-byte aligned, the matrices 8
    for name in names:
        if name not in ("colors", "rgb"):
            assert fuse(**{name: NULL}) == -1, name
    assert fuse(colors=NULL) == -1 and fuse(rgb=NULL) == -1
    for name in ("depth", "colors", "K", "R", "T", "pairs", "mat", "merged", "xyz", "rgb"):
        assert fuse(**{name: ODD}) == -1 and fuse(**{name: ctypes.c_void_p(0x1002)}) == -1, name
    assert fuse(mat=ctypes.c_void_p(0x1004)) == -1
    # S in 1..64, thresholds finite and > 0, dimensions
    for s in (0, -1, 65, 1000):
        assert fuse(s=s) == -1, s
    for v in (0.0, -1.0, INF, -INF, NAN):
        assert fuse(px=v) == -1 and fuse(rel=v) == -1, v
    for kw in ({"h": 0}, {"w": 0}, {"h": -4, "w": -4}, {"n": 0}, {"n": -1}):
        assert fuse(**kw) == -1, kw
    # N h w or N S at or past 2^31
    for n, h, w in ((1, 32768, 65536), (2, 32768, 32768), (49, 8192, 8192), (2 ** 20, 64, 32), (1, 2 ** 31 - 1, 2)):
        assert fuse(n=n, h=h, w=w) == -3, (n, h, w)
    assert fuse(n=2 ** 30, s=2, h=1, w=1) == -3
    with pytest.raises(_lib.MVSLibraryError):
        _lib.check(fuse(px=NAN), "mvs_fuse_views_fwd")


def test_op_schema_and_fake_kernel():
    ops = torch.ops.mvs_fusion
    assert str(ops.fuse_views.default._schema) == \
        ("mvs_fusion::fuse_views(Tensor depth, Tensor mask, Tensor? colors, Tensor K, Tensor R, Tensor T, "
         "Tensor pairs, Tensor matrices, float px_thresh, float rel_thresh) -> (Tensor, Tensor, Tensor, Tensor)")
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    args = (m(5, 3, 3), m(5, 3, 3), m(5, 3), m(5, 4, dtype=torch.int32), m(5, 4, 24, dtype=torch.float64), 1.0, 0.01)
    for colors in (None, m(5, 3, 17, 40)):
        em, cnt, xyz, rgb = ops.fuse_views(m(5, 1, 17, 40), m(5, 1, 17, 40, dtype=torch.bool), colors, *args)
        assert em.shape == cnt.shape == (5, 17, 40) and em.dtype == torch.bool and cnt.dtype == torch.int32
        assert xyz.shape == (5, 17, 40, 3) and xyz.dtype == torch.float32
        assert rgb.shape == ((0,) if colors is None else (5, 17, 40, 3)) and rgb.dtype == torch.float32
        assert not any(t.requires_grad for t in (em, cnt, xyz, rgb))


def test_no_cpu_kernel_and_host_side_checks():
    from mvs_amd import _lib, fusion
    depth = torch.full((2, 1, 3, 4), 500.0)
    K, R, T = torch.eye(3).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3, 1)
    with pytest.raises(_lib.MVSLibraryError):
        fusion.fused_point_cloud(depth, depth > 0, K, R, T, [[1], [0]])
    with pytest.raises(_lib.MVSLibraryError):
        fusion.fuse_views_op(depth, depth > 0, None, K, R, T.reshape(2, 3), torch.tensor([[1], [0]], dtype=torch.int32),
                             torch.zeros(2, 1, 24, dtype=torch.float64), 1.0, 0.01)
    for pairs in ([[1], [2]], [[-2], [0]], [[1], [0], [1]], [[1] * 65, [0]], torch.tensor([[1.0], [0.0]])):
        with pytest.raises(ValueError):
            fusion.fused_point_cloud(depth, depth > 0, K, R, T, pairs)


@pytest.mark.parametrize("case", fusion_cases.SCENES, ids=lambda c: "%dx%d-N%d-S%d" % c)
def test_restatement_meets_its_own_conditions(case):
    """What the GPU tests rely on, checked without a GPU: taint on at most 0.1 % of a scene's pixels (none under
    1000 pixels); the first view emits what its mask keeps; the restatement itself de-duplicates (the counts are
    those of the numpy prototype the rule was written with); a pixel is emitted only where kept, merges at most its
    non-empty slots, and a pixel that is not emitted holds zeros."""
    import fusion_ref
    sc = fused_cloud_ref.fused_scene(*case)
    taint, em, mask = sc["taint"], sc["emitted"], sc["mask"][:, 0]
    assert taint.mean() <= 1e-3 and (taint.size >= 1000 or not taint.any()), (case, taint.mean())
    assert np.array_equal(em[0], mask[0])
    assert not (em & ~mask).any()
    slots = fusion_ref.non_empty_slots(sc["table"]).reshape(-1, 1, 1)
    assert (sc["n_merged"] <= slots).all() and (sc["n_merged"][~em] == 0).all()
    assert (sc["xyz"][~em] == 0).all() and (sc["rgb"][~em] == 0).all()
    print("%s: emitted %d of %d kept, per view %s, taint %d" % (case, em.sum(), mask.sum(),
                                                                 em.reshape(len(em), -1).sum(1).tolist(), taint.sum()))
    if case in ((128, 160, 5, 4), (17, 40, 5, 10)):
        assert em.sum() < 0.35 * mask.sum(), (case, int(em.sum()), int(mask.sum()))
    if case in EMITTED_KEPT and not taint.any():
        assert (int(em.sum()), int(mask.sum())) == EMITTED_KEPT[case], case


def test_restatement_without_colours_and_reversed_pairs():
    sc = fused_cloud_ref.fused_scene(9, 33, 5, 4)
    em, cnt, xyz, rgb, taint = fused_cloud_ref.fuse(sc["depth"], sc["mask"], None, sc["K"], sc["R"], sc["T"],
                                                    sc["table"])
    assert rgb is None and np.array_equal(em, sc["emitted"]) and np.array_equal(cnt, sc["n_merged"])
    assert np.array_equal(xyz, sc["xyz"]) and np.array_equal(taint, sc["taint"])
    assert fused_cloud_ref.reversed_pairs([[1, 2], [0, -1], []], 3) == [[], [2, -1], [1, 0]]
    col = fused_cloud_ref.scene_colors(5, 9, 33)
    assert col.dtype == np.float32 and 0.1 <= col.min() < col.max() <= 0.9
    assert all(np.ptp(col, axis=a).min() > 0 for a in (0, 1)) and np.ptp(col, axis=3).min() > 0
