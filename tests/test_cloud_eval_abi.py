"""CPU: cloud evaluation (include/fusion/mvs_cloud_eval.h, mvs_amd.cloud_eval, mvs_amd.fusion.read_ply) -- header,
exports and bindings in sync, the cell-table size query, every refusal before any launch (dimensions and fake
pointers only: no memory is touched), the ops' schemas and fake kernels, the host-side argument checks, read_ply, and
the float64 restatement's own conditions on the clouds the GPU tests use.  No kernel is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_eval_ref as ref
from conftest import REPO

HEADER = os.path.join(REPO, "include", "fusion", "mvs_cloud_eval.h")
NAMES = ("mvs_cloud_cell_table_bytes", "mvs_cloud_cell_keys", "mvs_cloud_cell_ranges", "mvs_cloud_nearest")
NULL, FAKE, ODD = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001)
C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong}
INF, NAN = float("inf"), float("nan")
BAD, BIG = -1, -3                                    # MVS_ERR_INVALID_ARGUMENT, MVS_ERR_TOO_LARGE


def _header_signatures():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^\s*(int|size_t)\s+(mvs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        types = [ctypes.c_void_p if "*" in a else C_TYPES[" ".join(a.replace("const ", "").split()[:-1])]
                 for a in args.split(",")]
        out[name] = (C_TYPES[res], types)
    return out


def test_header_exports_and_bindings():
    from mvs_amd import _build, _lib, cloud_eval
    lib = _lib.load()
    declared = _header_signatures()
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.CLOUD_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        for table in (_lib.SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.LOSS_SIGNATURES, _lib.FILTER_SIGNATURES,
                      _lib.FUSE_SIGNATURES, _lib.LAUNCH_SIGNATURES):
            assert name not in table
        res, args = _lib.CLOUD_SIGNATURES[name]
        assert (res, list(args)) == declared[name], name
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 24                   # additive: not bumped
    assert HEADER in [os.path.abspath(p) for p in _build.HEADERS]
    assert any(os.path.basename(p) == "cloud_nn.hip" for p in _build.SOURCES)
    assert "cloud_nn.hip" not in _build.SOURCE_FLAGS                         # default build flags
    text = open(HEADER).read()
    assert "#define MVS_CLOUD_MAX_CELLS (1 << 27)" in text and "#define MVS_CLOUD_MAX_RINGS 64" in text
    assert (_lib.CLOUD_MAX_CELLS, _lib.CLOUD_MAX_RINGS) == (1 << 27, 64)
    for op in ("cell_keys", "cell_ranges", "nearest"):
        assert hasattr(torch.ops.mvs_cloud, op)
        assert not hasattr(torch.ops.mvs, op) and not hasattr(torch.ops.mvs_fusion, op)
    assert all(callable(getattr(cloud_eval, f)) for f in ("CloudIndex", "nearest_distance", "evaluate_cloud"))
    for word in ("observation mask", "ground plane", "0.2 mm"):
        assert word in " ".join(cloud_eval.evaluate_cloud.__doc__.split()), word
    assert "synchronis" in cloud_eval.CloudIndex.__doc__


def test_cell_table_bytes():
    from mvs_amd import _lib
    lib = _lib.load()
    for dims in ((1, 1, 1), (3, 5, 7), (512, 512, 512), (1 << 27, 1, 1), (1, 1 << 13, 1 << 14)):
        assert lib.mvs_cloud_cell_table_bytes(*dims) == 4 * (dims[0] * dims[1] * dims[2] + 1), dims
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), ((1 << 27) + 1, 1, 1), (513, 512, 512), (1 << 16, 1 << 16, 1),
                 (1 << 30, 1 << 30, 1 << 30), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (1 << 20, 1 << 20, 1 << 24)):
        assert lib.mvs_cloud_cell_table_bytes(*dims) == 0, dims


def test_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()
    grid = dict(ox=0.0, oy=0.0, oz=0.0, cell=1.0, nx=4, ny=4, nz=4)
    order = ("ox", "oy", "oz", "cell", "nx", "ny", "nz")

    def keys(points=FAKE, n=10, out=FAKE, **kw):
        g = dict(grid, **kw)
        return lib.mvs_cloud_cell_keys(points, n, *[g[k] for k in order], out, NULL)

    def ranges(sorted_keys=FAKE, n=10, ncells=64, start=FAKE):
        return lib.mvs_cloud_cell_ranges(sorted_keys, n, ncells, start, NULL)

    names = ("query", "order", "targets", "tindex", "start", "dist", "index")

    def nearest(m=10, g=10, max_dist=2.0, **kw):
        p = {k: kw.pop(k, FAKE) for k in names}
        gr = dict(grid, **kw)
        return lib.mvs_cloud_nearest(p["query"], p["order"], m, p["targets"], p["tindex"], g, p["start"],
                                     *[gr[k] for k in order], max_dist, p["dist"], p["index"], NULL)

    # pointers: non-null, 4-byte aligned
    for bad in (NULL, ODD, ctypes.c_void_p(0x1002)):
        assert keys(points=bad) == BAD and keys(out=bad) == BAD
        assert ranges(sorted_keys=bad) == BAD and ranges(start=bad) == BAD
        for name in names:
            assert nearest(**{name: bad}) == BAD, name
    # counts: negative, at or past the index width
    for call in (lambda v: keys(n=v), lambda v: ranges(n=v), lambda v: ranges(ncells=v), lambda v: nearest(m=v),
                 lambda v: nearest(g=v)):
        assert call(-1) == BAD and call(-2 ** 40) == BAD
        assert call(2 ** 31) == BIG and call(2 ** 40) == BIG
    assert ranges(ncells=0) == BAD and ranges(ncells=(1 << 27) + 1) == BAD and ranges(ncells=2 ** 31 - 1) == BAD
    # the grid: cell and max_dist finite and > 0, a finite origin, dimensions >= 1, at most 2^27 cells, 64 rings
    for call in (keys, nearest):
        for v in (0.0, -1.0, INF, -INF, NAN):
            assert call(cell=v) == BAD, v
        for v in (INF, -INF, NAN):
            assert call(ox=v) == BAD and call(oy=v) == BAD and call(oz=v) == BAD
        for kw in ({"nx": 0}, {"ny": -3}, {"nz": 0}, {"nx": (1 << 27) + 1, "ny": 1, "nz": 1},
                   {"nx": 513, "ny": 512, "nz": 512}):
            assert call(**kw) == BAD, kw
        for kw in ({"nx": 1 << 16, "ny": 1 << 16}, {"nx": 2 ** 31 - 1, "ny": 2 ** 31 - 1, "nz": 2 ** 31 - 1},
                   {"nx": 1 << 11, "ny": 1 << 10, "nz": 1 << 10}):
            assert call(**kw) == BIG, kw
    for v in (0.0, -1.0, INF, -INF, NAN):
        assert nearest(max_dist=v) == BAD, v
    assert nearest(max_dist=64.5) == BAD and nearest(max_dist=20.0, cell=0.3) == BAD and nearest(max_dist=1e300) == BAD
    # nothing to do: accepted without a launch
    assert keys(n=0) == 0 and nearest(m=0) == 0 and nearest(m=0, max_dist=64.0) == 0
    with pytest.raises(_lib.MVSLibraryError):
        _lib.check(nearest(max_dist=NAN), "mvs_cloud_nearest")


def test_op_schemas_and_fake_kernels():
    ops = torch.ops.mvs_cloud
    assert str(ops.cell_keys.default._schema) == \
        ("mvs_cloud::cell_keys(Tensor points, float ox, float oy, float oz, float cell, SymInt nx, SymInt ny, "
         "SymInt nz) -> Tensor")
    assert str(ops.cell_ranges.default._schema) == "mvs_cloud::cell_ranges(Tensor sorted_keys, SymInt ncells) -> Tensor"
    assert str(ops.nearest.default._schema) == \
        ("mvs_cloud::nearest(Tensor query, Tensor query_order, Tensor targets, Tensor target_index, Tensor cell_start, "
         "float ox, float oy, float oz, float cell, SymInt nx, SymInt ny, SymInt nz, float max_dist) "
         "-> (Tensor, Tensor)")
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    i32 = torch.int32
    keys = ops.cell_keys(m(70, 3), 0.0, 0.0, 0.0, 1.5, 3, 4, 5)
    assert keys.shape == (70,) and keys.dtype == i32
    start = ops.cell_ranges(m(70, dtype=i32), 60)
    assert start.shape == (61,) and start.dtype == i32
    dist, index = ops.nearest(m(33, 3), m(33, dtype=i32), m(70, 3), m(70, dtype=i32), m(61, dtype=i32), 0.0, 0.0, 0.0,
                              1.5, 3, 4, 5, 20.0)
    assert dist.shape == index.shape == (33,) and dist.dtype == torch.float32 and index.dtype == i32
    assert not dist.requires_grad and not index.requires_grad


def test_no_cpu_kernel_and_host_side_checks():
    from mvs_amd import _lib, cloud_eval
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for call in (lambda: cloud_eval.CloudIndex(a, 1.0), lambda: cloud_eval.nearest_distance(a, b, 1.0),
                 lambda: cloud_eval.evaluate_cloud(a, b), lambda: cloud_eval.cell_keys_op(a, 0.0, 0.0, 0.0, 1.0, 1, 1, 1),
                 lambda: cloud_eval.cell_ranges_op(torch.zeros(4, dtype=torch.int32), 4)):
        with pytest.raises(_lib.MVSLibraryError):
            call()
    # shapes other than [., 3], a dtype other than fp32
    for bad in (torch.rand(10, 2), torch.rand(10, 4), torch.rand(3), torch.rand(2, 5, 3), torch.rand(10, 3).double(),
                torch.rand(10, 3).half(), torch.zeros(10, 3, dtype=torch.int32), [[0.0, 0.0, 0.0]]):
        for call in (lambda: cloud_eval.CloudIndex(bad, 1.0), lambda: cloud_eval.nearest_distance(bad, a, 1.0),
                     lambda: cloud_eval.nearest_distance(a, bad, 1.0), lambda: cloud_eval.evaluate_cloud(bad, a),
                     lambda: cloud_eval.evaluate_cloud(a, bad)):
            with pytest.raises(ValueError):
                call()
    # tau outside (0, max_dist]; max_dist and cell finite and > 0
    for taus in ((20.5,), (1.0, 0.0), (-1.0,), (NAN,), (INF,)):
        with pytest.raises(ValueError, match="max_dist"):
            cloud_eval.evaluate_cloud(a, b, 20.0, taus)
    for v in (0.0, -2.0, INF, NAN):
        with pytest.raises(ValueError):
            cloud_eval.CloudIndex(a, v)
        with pytest.raises(ValueError):
            cloud_eval.CloudIndex(a, 1.0, cell=v)
        with pytest.raises(ValueError):
            cloud_eval.evaluate_cloud(a, b, v)
    # an explicit cell past a limit names it
    with pytest.raises(ValueError, match="ring limit"):
        cloud_eval.CloudIndex(a, 20.0, cell=0.3)
    with pytest.raises(ValueError, match="ring limit"):
        cloud_eval.choose_grid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 10, 20.0, 0.3)
    with pytest.raises(ValueError, match="cell limit"):
        cloud_eval.choose_grid((0.0, 0.0, 0.0), (600.0, 600.0, 600.0), 10, 20.0, 1.0)
    assert cloud_eval.choose_grid((0.0, 0.0, 0.0), (511.5, 511.5, 511.5), 10, 20.0, 1.0) == (1.0, (512, 512, 512))
    assert cloud_eval.choose_grid((1.0, 2.0, 3.0), (1.0, 2.0, 3.0), 5, 20.0) == (20.0 / 64, (1, 1, 1))


def test_default_grid_stays_within_the_limits():
    from mvs_amd import _lib, cloud_eval
    for lo, hi, count, max_dist in (((0.0,) * 3, (300.0, 300.0, 50.0), 10 ** 6, 20.0),
                                    ((0.0,) * 3, (1e5, 1e5, 1e5), 10 ** 7, 20.0),
                                    ((-5.0,) * 3, (5.0, 5.0, 5.0), 100, 2000.0),
                                    ((0.0,) * 3, (1e4, 0.0, 0.0), 50, 1.0), ((0.0,) * 3, (300.0, 300.0, 300.0), 1, 20.0)):
        cell, dims = cloud_eval.choose_grid(lo, hi, count, max_dist)
        assert dims[0] * dims[1] * dims[2] <= _lib.CLOUD_MAX_CELLS and min(dims) >= 1, (lo, hi, dims)
        assert np.ceil(max_dist / cell) <= _lib.CLOUD_MAX_RINGS
        assert dims == cloud_eval.grid_dims(lo, hi, cell)
        assert _lib.load().mvs_cloud_cell_table_bytes(*dims) == 4 * (dims[0] * dims[1] * dims[2] + 1)
    # a surface of 10^6 points over 300 x 300: POINTS_PER_CELL per occupied cell
    cell, _ = cloud_eval.choose_grid((0.0,) * 3, (300.0, 300.0, 50.0), 10 ** 6, 20.0)
    assert abs(cell * cell * 10 ** 6 / 9e4 - cloud_eval.POINTS_PER_CELL) < 1e-9


# ---- read_ply ----------------------------------------------------------------------------------------
def test_read_ply_round_trip_of_write_ply(tmp_path):
    from mvs_amd import fusion
    rng = np.random.default_rng(3)
    pts = (rng.normal(0.0, 300.0, (257, 3))).astype(np.float32)
    col = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    path = str(tmp_path / "a.ply")
    fusion.write_ply(path, pts, col)
    p, c = fusion.read_ply(path)
    assert p.dtype == np.float32 and c.dtype == np.uint8 and np.array_equal(p, pts) and np.array_equal(c, col)
    fusion.write_ply(path, torch.from_numpy(pts))
    p, c = fusion.read_ply(path)
    assert c is None and np.array_equal(p, pts) and p.shape == (257, 3)
    fusion.write_ply(path, np.zeros((0, 3), np.float32))
    p, c = fusion.read_ply(path)
    assert p.shape == (0, 3) and p.dtype == np.float32 and c is None
    assert "read_ply" in fusion.__doc__


def _write(path, header, body):
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(body)
    return str(path)


def test_read_ply_formats(tmp_path):
    from mvs_amd import fusion
    # ascii, with a comment, colours, an extra property and a trailing face element
    path = _write(tmp_path / "ascii.ply",
                  ["ply", "format ascii 1.0", "comment made by hand", "element vertex 3", "property float x",
                   "property float y", "property float z", "property float quality", "property uchar red",
                   "property uchar green", "property uchar blue", "element face 1",
                   "property list uchar int vertex_indices"],
                  b"0 1.5 -2 0.5 255 0 7\n1e2 2.25 3 0.25 1 2 3\n-4 5 6.125 0 9 8 7\n3 0 1 2\n")
    p, c = fusion.read_ply(path)
    assert np.array_equal(p, np.array([[0, 1.5, -2], [100, 2.25, 3], [-4, 5, 6.125]], np.float32))
    assert np.array_equal(c, np.array([[255, 0, 7], [1, 2, 3], [9, 8, 7]], np.uint8))
    # binary: double coordinates in another order, extra properties of several types between them, faces after
    dtype = np.dtype([("nx", "<f4"), ("z", "<f8"), ("flag", "i1"), ("x", "<f8"), ("count", "<u2"), ("y", "<f8"),
                      ("id", "<i4")])
    rec = np.zeros(5, dtype)
    rng = np.random.default_rng(5)
    for k in "xyz":
        rec[k] = rng.normal(0.0, 500.0, 5)
    rec["id"] = np.arange(5)
    faces = np.array([3, 0, 0, 0, 0], np.uint8).tobytes() * 3
    path = _write(tmp_path / "double.ply",
                  ["ply", "format binary_little_endian 1.0", "element vertex 5", "property float nx",
                   "property double z", "property char flag", "property float64 x", "property ushort count",
                   "property double y", "property int32 id", "element face 3",
                   "property list uchar int vertex_indices"], rec.tobytes() + faces)
    p, c = fusion.read_ply(path)
    assert c is None and p.dtype == np.float32
    assert np.array_equal(p, np.stack([rec["x"], rec["y"], rec["z"]], 1).astype(np.float32))


def test_read_ply_refusals(tmp_path):
    from mvs_amd import fusion
    xyz = ["property float x", "property float y", "property float z"]
    body = np.arange(6, dtype="<f4").tobytes()
    ok = _write(tmp_path / "ok.ply", ["ply", "format binary_little_endian 1.0", "element vertex 2"] + xyz, body)
    assert fusion.read_ply(ok)[0].tolist() == [[0, 1, 2], [3, 4, 5]]
    cases = {
        "list": (["ply", "format binary_little_endian 1.0", "element vertex 2"] + xyz +
                 ["property list uchar int neighbours"], body, "list"),
        "big": (["ply", "format binary_big_endian 1.0", "element vertex 2"] + xyz, body, "binary_big_endian"),
        "short": (["ply", "format binary_little_endian 1.0", "element vertex 2"] + xyz, body[:-1], "ends before"),
        "short_ascii": (["ply", "format ascii 1.0", "element vertex 2"] + xyz, b"0 1 2\n3 4\n", "ends before"),
        "face_first": (["ply", "format ascii 1.0", "element face 0", "property list uchar int vertex_indices",
                        "element vertex 2"] + xyz, b"0 1 2\n3 4 5\n", "first element"),
        "no_z": (["ply", "format ascii 1.0", "element vertex 2"] + xyz[:2], b"0 1\n3 4\n", "x, y and z"),
        "int_x": (["ply", "format ascii 1.0", "element vertex 2", "property int x"] + xyz[1:], b"0 1 2\n3 4 5\n",
                  "float or double"),
    }
    for name, (header, data, match) in cases.items():
        with pytest.raises(ValueError, match=match):
            fusion.read_ply(_write(tmp_path / (name + ".ply"), header, data))
    with pytest.raises(ValueError, match="not a PLY"):
        fusion.read_ply(_write(tmp_path / "not.ply", ["plx"], b""))


# ---- the restatement ---------------------------------------------------------------------------------
def test_restatement_on_known_answers():
    q = np.array([[0, 0, 0], [100, 0, 0], [np.nan, 0, 0], [3, 4, 0]], np.float32)
    t = np.array([[3, 4, 0], [0, 0, 5], [-5, 0, 0], [np.inf, 0, 0], [12, 16, 0], [0, 0, 0]], np.float32)
    dist, index, best, flag = ref.nearest(q, t, 20.0)
    assert dist.tolist() == [0.0, INF, INF, 0.0] and index.tolist() == [5, -1, -1, 0] and not flag.any()
    dist, index, best, flag = ref.nearest(q, t[:5], 20.0)
    assert dist.tolist() == [5.0, INF, INF, 0.0] and index.tolist() == [0, -1, -1, 0] and best[0] == 25.0
    assert not flag.any()                 # (12, 16, 0), at exactly max_dist from query 0, is accepted and not the best
    dist, index, _, flag = ref.nearest(q[:1], t[4:5], 20.0)
    assert dist[0] == 20.0 and index[0] == 0 and flag[0]
    dist, index, _, flag = ref.nearest(q[:1], t[4:5] + np.float32([0, 0, 1]), 20.0)
    assert dist[0] == INF and index[0] == -1 and not flag[0]
    dist, index, _, _ = ref.nearest(q, np.zeros((0, 3), np.float32), 20.0)
    assert np.isinf(dist).all() and (index == -1).all()
    assert ref.nearest(np.zeros((0, 3), np.float32), t, 20.0)[0].shape == (0,)


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: "%s%d-%s%d" % c)
def test_restatement_meets_its_own_conditions(case):
    """What the GPU tests rely on, checked without a GPU: near-the-gate flags on at most 0.1 % of a case's queries,
    none for a cloud under 1000 points, and with these seeds none at all; the clouds sit in DTU's world range."""
    query, target = ref.case_clouds(case)
    assert query.shape == (case[1], 3) and target.shape == (case[3], 3) and query.dtype == np.float32
    assert case[1] in ref.SIZES and case[3] in ref.SIZES
    dist, index, best, flag = ref.case_reference(case)
    assert flag.mean() <= 1e-3 and (min(case[1], case[3]) >= 1000 or not flag.any())
    assert not flag.any()
    assert np.array_equal(index >= 0, np.isfinite(dist)) and (dist[index >= 0] <= ref.MAX_DIST).all()
    assert np.abs(query).max() > 100.0 and np.abs(target).max() > 100.0
    print("%s: %d of %d found, %d flagged" % (case, int((index >= 0).sum()), len(index), int(flag.sum())))


def test_cases_cover_every_size_on_both_sides():
    assert {c[1] for c in ref.CASES} == set(ref.SIZES) == {c[3] for c in ref.CASES}
    assert {c[0] for c in ref.CASES} == {c[2] for c in ref.CASES} == {"sheet", "box"}
