"""CPU: depth-map filtering and fusion (include/fusion/mvs_depth_filter.h, mvs_amd/fusion.py) -- header, exports and
bindings in sync, every refusal before any launch (dimensions and fake pointers only: no memory is touched), the
matrix-buffer query, the mvs_fusion op schemas and fake kernels, the host-side argument checks, write_ply, and the
float64 restatement's own decision margin on the plane scenes the GPU tests use.  No kernel is launched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fusion_ref
from conftest import REPO

HEADER = os.path.join(REPO, "include", "fusion", "mvs_depth_filter.h")
NAMES = ("mvs_photometric_confidence_fwd", "mvs_view_pair_matrices_bytes", "mvs_view_pair_matrices",
         "mvs_geometric_consistency_fwd", "mvs_backproject_fwd")
NULL, FAKE, ODD = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
C_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
INF, NAN = float("inf"), float("nan")


def _header_signatures():
    """name -> (restype, argtypes) read from the header's declarations: pointers are void*, the rest by name."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^\s*(int|size_t)\s+(mvs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (C_TYPES[res], types)
    return out


def test_package_exports_fusion():
    import mvs_amd
    from mvs_amd import fusion
    from mvs_amd.model import MVSNet
    assert mvs_amd.fusion is fusion and "fusion" in mvs_amd.__all__
    for name in ("photometric_confidence", "geometric_consistency", "filter_depth", "point_cloud", "write_ply"):
        assert callable(getattr(fusion, name)), name
    fwd = inspect.signature(MVSNet.forward)
    assert list(inspect.signature(MVSNet.forward_with_confidence).parameters) == list(fwd.parameters)
    one = inspect.signature(MVSNet._forward_one).parameters
    assert list(one)[:len(fwd.parameters)] == list(fwd.parameters)
    assert one["with_confidence"].default is False               # the present behaviour is the default
    # four ops, in a namespace of their own; the drop-in namespace gains none
    for name in ("photometric_confidence", "view_pair_matrices", "geometric_consistency", "backproject"):
        assert hasattr(torch.ops.mvs_fusion, name), name
        assert not hasattr(torch.ops.mvs, name), name


def test_header_exports_and_bindings():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    declared = _header_signatures()
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.FILTER_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name not in _lib.SIGNATURES and name not in _lib.TRAIN_SIGNATURES and name not in _lib.LOSS_SIGNATURES
        res, args = _lib.FILTER_SIGNATURES[name]
        assert (res, list(args)) == declared[name], name
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 24                   # additive: neither is bumped
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1
    assert HEADER in [os.path.abspath(p) for p in _build.HEADERS]
    assert any(os.path.basename(p) == "depth_filter.hip" for p in _build.SOURCES)
    assert "depth_filter.hip" not in _build.SOURCE_FLAGS                     # default build flags
    assert re.search(r"#define\s+MVS_FILTER_MAX_SLOTS\s+64\b", open(HEADER).read()) and _lib.FILTER_MAX_SLOTS == 64


def test_pair_matrix_bytes():
    from mvs_amd import _lib
    lib = _lib.load()
    for n in (1, 2, 5, 49, 1000):
        for s in (1, 4, 10, 64):
            assert lib.mvs_view_pair_matrices_bytes(n, s) == n * s * 24 * 8
    for n, s in ((0, 4), (-1, 4), (5, 0), (5, -2), (5, 65), (2 ** 30, 2)):
        assert lib.mvs_view_pair_matrices_bytes(n, s) == 0, (n, s)


def test_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()

    def conf(prob=FAKE, depth=FAKE, db=FAKE, batch=2, d=5, h=5, w=7, out=FAKE):
        return lib.mvs_photometric_confidence_fwd(prob, depth, db, batch, d, h, w, out, NULL)

    def mats(K=FAKE, R=FAKE, T=FAKE, pairs=FAKE, n=5, s=4, out=FAKE):
        return lib.mvs_view_pair_matrices(K, R, T, pairs, n, s, out, NULL)

    def geo(depth=FAKE, pairs=FAKE, mat=FAKE, n=5, s=4, h=5, w=7, px=1.0, rel=0.01, cnt=FAKE, avg=FAKE):
        return lib.mvs_geometric_consistency_fwd(depth, pairs, mat, n, s, h, w, px, rel, cnt, avg, NULL)

    def back(depth=FAKE, K=FAKE, R=FAKE, T=FAKE, n=5, h=5, w=7, out=FAKE):
        return lib.mvs_backproject_fwd(depth, K, R, T, n, h, w, out, NULL)

    # pointers: non-null, 4-byte aligned (the matrices 8-byte)
    for fn, names in ((conf, ("prob", "depth", "db", "out")), (mats, ("K", "R", "T", "pairs", "out")),
                      (geo, ("depth", "pairs", "mat", "cnt", "avg")), (back, ("depth", "K", "R", "T", "out"))):
        for name in names:
            assert fn(**{name: NULL}) == -1 and fn(**{name: ODD}) == -1, (fn.__name__, name)
    assert mats(out=ctypes.c_void_p(0x1004)) == -1 and geo(mat=ctypes.c_void_p(0x1004)) == -1
    # D >= 2
    for d in (1, 0, -3):
        assert conf(d=d) == -1, d
    # S in 1..64
    for s in (0, -1, 65, 1000):
        assert mats(s=s) == -1 and geo(s=s) == -1, s
    # thresholds finite and > 0
    for v in (0.0, -1.0, INF, -INF, NAN):
        assert geo(px=v) == -1 and geo(rel=v) == -1, v
    # dimensions
    for kw in ({"h": 0}, {"w": 0}, {"h": -4, "w": -4}):
        assert conf(**kw) == -1 and geo(**kw) == -1 and back(**kw) == -1, kw
    for kw in ({"n": 0}, {"n": -1}):
        assert mats(**kw) == -1 and geo(**kw) == -1 and back(**kw) == -1, kw
    assert conf(batch=0) == -1 and conf(batch=-2) == -1
    # N h w (B h w for the confidence) at or past 2^31
    for n, h, w in ((1, 32768, 65536), (2, 32768, 32768), (49, 8192, 8192), (2 ** 20, 64, 32), (1, 2 ** 31 - 1, 2)):
        assert conf(batch=n, h=h, w=w) == -3 and geo(n=n, h=h, w=w) == -3 and back(n=n, h=h, w=w) == -3, (n, h, w)
    assert mats(n=2 ** 30, s=2) == -3                          # N S at or past 2^31
    with pytest.raises(_lib.MVSLibraryError):
        _lib.check(geo(px=NAN), "mvs_geometric_consistency_fwd")


def test_ops_have_no_cpu_kernel_and_check_their_arguments():
    from mvs_amd import _lib, fusion
    depth = torch.full((2, 1, 3, 4), 500.0)
    K, R, T = torch.eye(3).repeat(2, 1, 1), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3, 1)
    with pytest.raises(_lib.MVSLibraryError):
        fusion.photometric_confidence(torch.rand(2, 1, 5, 3, 4), depth, torch.rand(1, 5))
    with pytest.raises(_lib.MVSLibraryError):
        fusion.geometric_consistency(depth, K, R, T, [[1], [0]])
    with pytest.raises(_lib.MVSLibraryError):
        fusion.backproject(depth, K, R, T)
    with pytest.raises(_lib.MVSLibraryError):
        fusion.view_pair_matrices(K, R, T.reshape(2, 3), torch.tensor([[1], [0]], dtype=torch.int32))
    with pytest.raises(_lib.MVSLibraryError):
        fusion.point_cloud(depth, depth > 0, K, R, T)
    # a pair index outside [-1, N): refused on the host, before anything else
    for pairs in ([[1], [2]], [[-2], [0]], torch.tensor([[1, -1], [0, 5]]), [[1, 0], [7]]):
        with pytest.raises(ValueError):
            fusion.geometric_consistency(depth, K, R, T, pairs)
    with pytest.raises(ValueError):
        fusion.geometric_consistency(depth, K, R, T, [[1], [0], [1]])       # three rows for two views
    with pytest.raises(ValueError):
        fusion.geometric_consistency(depth, K, R, T, [[1] * 65, [0]])       # more than 64 slots
    with pytest.raises(ValueError):
        fusion.geometric_consistency(depth, K, R, T, torch.tensor([[1.0], [0.0]]))


def test_pair_table_pads_ragged_lists():
    from mvs_amd.fusion import pair_table
    t = pair_table([[1, 2, 3], [0], [], [3, 0]], 4)
    assert t.dtype == torch.int32 and t.device.type == "cpu"
    assert t.tolist() == [[1, 2, 3], [0, -1, -1], [-1, -1, -1], [3, 0, -1]]
    assert pair_table([[]], 1).tolist() == [[-1]]                            # never zero slots
    assert pair_table(torch.tensor([[1, -1], [0, 1]], dtype=torch.int64), 2).tolist() == [[1, -1], [0, 1]]
    assert pair_table(torch.zeros((3, 0), dtype=torch.int64), 3).tolist() == [[-1]] * 3
    assert np.array_equal(fusion_ref.pad_pairs([[1, 2, 3], [0], [], [3, 0]]), t.numpy())


def test_op_schemas_and_fake_kernels():
    ops = torch.ops.mvs_fusion
    assert str(ops.photometric_confidence.default._schema) == \
        "mvs_fusion::photometric_confidence(Tensor prob_volume, Tensor depth, Tensor d_batch) -> Tensor"
    assert str(ops.view_pair_matrices.default._schema) == \
        "mvs_fusion::view_pair_matrices(Tensor K, Tensor R, Tensor T, Tensor pairs) -> Tensor"
    assert str(ops.geometric_consistency.default._schema) == \
        ("mvs_fusion::geometric_consistency(Tensor depth, Tensor pairs, Tensor matrices, float px_thresh, "
         "float rel_thresh) -> (Tensor, Tensor)")
    assert str(ops.backproject.default._schema) == \
        "mvs_fusion::backproject(Tensor depth, Tensor K, Tensor R, Tensor T) -> Tensor"
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    conf = ops.photometric_confidence(m(3, 1, 48, 9, 33), m(3, 1, 9, 33), m(1, 48))
    assert conf.shape == (3, 1, 9, 33) and conf.dtype == torch.float32 and not conf.requires_grad
    mats = ops.view_pair_matrices(m(5, 3, 3), m(5, 3, 3), m(5, 3), m(5, 4, dtype=torch.int32))
    assert mats.shape == (5, 4, 24) and mats.dtype == torch.float64
    cnt, avg = ops.geometric_consistency(m(5, 1, 17, 40), m(5, 4, dtype=torch.int32),
                                         m(5, 4, 24, dtype=torch.float64), 1.0, 0.01)
    assert cnt.shape == avg.shape == (5, 1, 17, 40) and cnt.dtype == torch.int32 and avg.dtype == torch.float32
    xyz = ops.backproject(m(5, 1, 17, 40), m(5, 3, 3), m(5, 3, 3), m(5, 3))
    assert xyz.shape == (5, 17, 40, 3) and xyz.dtype == torch.float32
    # no autograd formula is registered, and the package's functions hand the ops detached tensors
    from mvs_amd import fusion
    conf = fusion.photometric_confidence(m(1, 1, 4, 2, 2).requires_grad_(True), m(1, 1, 2, 2), m(1, 4))
    assert conf.shape == (1, 1, 2, 2) and not conf.requires_grad


def _read_ply(path):
    raw = open(path, "rb").read()
    head, payload = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    count = int(lines[2].split()[2])
    assert lines[2] == "element vertex %d" % count
    kinds = {"float": "<f4", "uchar": "u1"}
    fields = [(ln.split()[2], kinds[ln.split()[1]]) for ln in lines[3:-1]]
    assert all(ln.startswith("property ") for ln in lines[3:-1])
    rec = np.frombuffer(payload, dtype=np.dtype(fields))
    assert rec.shape == (count,)
    return rec


def test_write_ply_round_trip(tmp_path):
    from mvs_amd.fusion import write_ply
    rng = np.random.default_rng(4)
    pts = (rng.standard_normal((37, 3)) * 300.0).astype(np.float32)
    col = rng.integers(0, 256, (37, 3)).astype(np.uint8)
    write_ply(str(tmp_path / "a.ply"), torch.from_numpy(pts), torch.from_numpy(col))
    rec = _read_ply(str(tmp_path / "a.ply"))
    assert rec.dtype.names == ("x", "y", "z", "red", "green", "blue") and rec.dtype.itemsize == 15
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), pts)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), col)
    write_ply(str(tmp_path / "b.ply"), pts)                                  # arrays, no colours
    rec = _read_ply(str(tmp_path / "b.ply"))
    assert rec.dtype.names == ("x", "y", "z") and np.array_equal(rec["y"], pts[:, 1])
    write_ply(str(tmp_path / "c.ply"), pts[:2], np.array([[0.0, 0.5, 1.0], [2.0, -1.0, 0.2]]))   # 0..1 floats
    rec = _read_ply(str(tmp_path / "c.ply"))
    assert [int(rec[k][0]) for k in ("red", "green", "blue")] == [0, 128, 255]
    assert [int(rec[k][1]) for k in ("red", "green", "blue")] == [255, 0, 51]
    write_ply(str(tmp_path / "d.ply"), np.zeros((0, 3), np.float32))         # an empty cloud is a valid file
    assert _read_ply(str(tmp_path / "d.ply")).shape == (0,)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "e.ply"), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "e.ply"), pts, col[:5])


def test_restatement_meets_its_own_margins_on_the_plane_scenes():
    """What the GPU tests rely on, checked without a GPU: on every scene the float64 restatement leaves at most
    0.1 % of the pixels near a decision (none below 1000 pixels), and on the larger maps it gives the full count on
    a majority of the interior pixels."""
    import fusion_cases
    for case in fusion_cases.SCENES:
        sc = fusion_cases.scene(*case)
        near = sc["near"]
        assert near.mean() <= 1e-3 and (near.size >= 1000 or not near.any()), (case, near.mean())
        if case in fusion_cases.FULL_COUNT:
            share = fusion_cases.full_count_share(sc)
            assert share > fusion_cases.FULL_COUNT_SHARE, (case, share)
