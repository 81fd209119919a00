"""CPU: the 2-D convolutions' backward in the training extension of the C ABI (include/train/mvs_region_train.h:
mvs_conv2d_wgrad_plan / _workspace_bytes / mvs_conv2d_wgrad / mvs_conv2d_dgrad) -- header, exports and bindings in
sync, every refusal before any launch (dimensions and fake pointers only: no memory is touched), the workspace and
plan queries against the formula mirrored here -- and the MVS_TRAIN_CONV2D_BWD switch (model.conv2d_bwd_mode).
No kernel is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TRAIN_HEADER = os.path.join(REPO, "include", "train", "mvs_region_train.h")
NAMES = ("mvs_conv2d_wgrad_plan", "mvs_conv2d_wgrad_workspace_bytes", "mvs_conv2d_wgrad", "mvs_conv2d_dgrad")
SHAPES = ((3, 8, 3, 1), (8, 8, 3, 1), (8, 16, 5, 2), (16, 16, 3, 1), (16, 32, 5, 2), (32, 32, 3, 1), (4, 32, 3, 1),
          (32, 1, 3, 1))
NULL, FAKE, ODD = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)


def _out(n, k, s):
    return (n + 2 * (k // 2) - k) // s + 1


def _plan(n, cin, cout, h, w, k, s):
    """The plan mirrored: 32 x 8 output tiles, at most 512 persistent workgroups = slots, a slot of
    [c_in][taps padded to 16][c_out padded to 16] floats."""
    tiles = n * -(-_out(h, k, s) // 8) * -(-_out(w, k, s) // 32)
    slots = min(tiles, 512)
    return tiles, slots, slots * cin * 16 * -(-(k * k) // 16) * 16 * -(-cout // 16) * 4


def test_header_exports_and_bindings():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(TRAIN_HEADER).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name) and name in _lib.TRAIN_SIGNATURES and name not in _lib.SIGNATURES
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1    # additive: not bumped
    assert any(os.path.basename(p) == "conv2d_bwd.hip" for p in _build.SOURCES)
    # built without packed fp32, like bn_train_bwd.hip
    assert _build.SOURCE_FLAGS["conv2d_bwd.hip"] == _build.SOURCE_FLAGS["bn_train_bwd.hip"]


def test_plan_and_workspace_queries_match_the_formula():
    from mvs_amd import _lib, conv2d_train
    lib = _lib.load()
    sizes = ((1, 1, 1), (1, 2, 3), (3, 9, 33), (2, 17, 40), (3, 7, 10), (1, 8, 9), (2, 500, 637), (12, 512, 640),
             (4, 128, 160))
    for cin, cout, k, s in SHAPES:
        for n, h, w in sizes:
            tiles, slots = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.mvs_conv2d_wgrad_plan(n, cin, cout, h, w, k, s, ctypes.byref(tiles), ctypes.byref(slots)) == 0
            want = _plan(n, cin, cout, h, w, k, s)
            assert (tiles.value, slots.value) == want[:2], (cin, cout, k, s, n, h, w)
            assert lib.mvs_conv2d_wgrad_workspace_bytes(n, cin, cout, h, w, k, s) == want[2]
            assert conv2d_train.wgrad_plan(n, cin, cout, h, w, k, s) == want[:2]
    # null outputs are allowed; the status is the launch's
    assert lib.mvs_conv2d_wgrad_plan(1, 3, 8, 4, 4, 3, 1, None, None) == 0
    # the encoder's full-resolution layers at cfg 2: 15360 tiles, 30 per persistent workgroup
    assert _plan(12, 3, 8, 512, 640, 3, 1)[:2] == (15360, 512)


def test_arguments_rejected_before_any_launch():
    from mvs_amd import _lib, conv2d_train
    lib = _lib.load()

    def wgrad(x=FAKE, gy=FAKE, n=2, shape=(8, 8, 3, 1), h=20, w=30, dw=FAKE, ws=FAKE):
        cin, cout, k, s = shape
        return lib.mvs_conv2d_wgrad(x, gy, n, cin, cout, h, w, k, s, dw, ws, NULL)

    def dgrad(gy=FAKE, wt=FAKE, n=2, shape=(8, 8, 3, 1), h=20, w=30, gx=FAKE):
        cin, cout, k, s = shape
        return lib.mvs_conv2d_dgrad(gy, wt, n, cin, cout, h, w, k, s, gx, NULL)

    def queries(n, shape, h, w):
        cin, cout, k, s = shape
        t = ctypes.c_int(-7)
        st = lib.mvs_conv2d_wgrad_plan(n, cin, cout, h, w, k, s, ctypes.byref(t), None)
        assert st == 0 or t.value == -7          # a refused plan writes nothing
        return st, lib.mvs_conv2d_wgrad_workspace_bytes(n, cin, cout, h, w, k, s)

    for name in ("x", "gy", "dw", "ws"):
        assert wgrad(**{name: NULL}) == -1 and wgrad(**{name: ODD}) == -1, name
    for name in ("gy", "wt", "gx"):
        assert dgrad(**{name: NULL}) == -1 and dgrad(**{name: ODD}) == -1, name
    # shapes, strides and kernel sizes without kernels; degenerate dimensions
    bad = [(8, 8, 3, 2), (8, 8, 5, 1), (8, 16, 5, 1), (8, 16, 3, 2), (16, 8, 3, 1), (1, 32, 3, 1), (3, 8, 1, 1),
           (32, 32, 3, 0), (32, 32, 7, 1), (0, 8, 3, 1), (64, 64, 3, 1)]
    for shape in bad:
        assert wgrad(shape=shape) == -1 and dgrad(shape=shape) == -1, shape
        assert queries(2, shape, 20, 30) == (-1, 0), shape
    for kw in ({"n": 0}, {"n": -1}, {"h": 0}, {"w": 0}):
        assert wgrad(**kw) == -1 and dgrad(**kw) == -1, kw
    # element counts of x or gy at or past 2^31
    wide = [(1, (8, 8, 3, 1), 16384, 16384),      # x and gy: 2^31 exactly
            (12, (3, 8, 3, 1), 8192, 8192),       # both
            (5, (3, 8, 3, 1), 8192, 8192),        # gy only (40 x 2^26), x is 15 x 2^26
            (3, (32, 1, 3, 1), 8192, 8192),       # x only
            (2, (16, 32, 5, 2), 65536, 65536),    # one plane past 2^31
            (2 ** 30, (8, 8, 3, 1), 2 ** 15, 2 ** 15)]   # the full product past 2^64
    for n, shape, h, w in wide:
        assert wgrad(n=n, shape=shape, h=h, w=w) == -3, (n, shape, h, w)
        assert dgrad(n=n, shape=shape, h=h, w=w) == -3, (n, shape, h, w)
        assert queries(n, shape, h, w) == (-3, 0)
        with pytest.raises(ValueError):
            conv2d_train.wgrad_plan(n, *shape[:2], h, w, *shape[2:])
    # just below: accepted by the queries (dimensions only)
    assert queries(1, (8, 8, 3, 1), 16384, 16383)[0] == 0
    # the input gradient's batch rides in grid.y; the weight gradient's does not
    assert dgrad(n=65536, shape=(32, 1, 3, 1), h=2, w=2) == -3
    assert queries(65536, (32, 1, 3, 1), 2, 2)[0] == 0


@pytest.mark.parametrize("value,want", [(None, "taps"), ("", "taps"), ("taps", "taps"), ("hip", "hip")])
def test_switch_parser(monkeypatch, value, want):
    from mvs_amd import model
    if value is None:
        monkeypatch.delenv("MVS_TRAIN_CONV2D_BWD", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_CONV2D_BWD", value)
    assert model.conv2d_bwd_mode() == want


@pytest.mark.parametrize("value", ["HIP", "1", "hip,taps", "s1", "on"])
def test_switch_parser_refuses_junk(monkeypatch, value):
    from mvs_amd import model
    monkeypatch.setenv("MVS_TRAIN_CONV2D_BWD", value)
    with pytest.raises(ValueError):
        model.conv2d_bwd_mode()


def test_no_other_switch_enables_it(monkeypatch):
    from mvs_amd import model
    monkeypatch.delenv("MVS_TRAIN_CONV2D_BWD", raising=False)
    for name in ("MVS_TRAIN_REGION_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_T2_BWD", "MVS_TRAIN_DECONV1", "MVS_TRAIN_BN",
                 "MVS_TRAIN_REGION_FWD"):
        monkeypatch.setenv(name, "hip")
    assert model.conv2d_bwd_mode() == "taps"


def test_routed_shapes_are_supported_shapes():
    import torch
    from mvs_amd import conv2d_train, ops
    assert set(conv2d_train.CONV2D_BWD_SHAPES) <= set(ops.CONV2D_SHAPES)
    assert len(set(conv2d_train.CONV2D_BWD_SHAPES)) == len(conv2d_train.CONV2D_BWD_SHAPES)
    assert set(SHAPES) == set(ops.CONV2D_SHAPES)
    # the two ops are torch.library ops of the training namespace; the drop-in namespace gains none
    assert hasattr(torch.ops.mvs_train, "conv2d_dgrad") and hasattr(torch.ops.mvs_train, "conv2d_wgrad")
    assert not hasattr(torch.ops.mvs, "conv2d_dgrad") and not hasattr(torch.ops.mvs, "conv2d_wgrad")
    # no CPU fallback
    from mvs_amd import _lib
    with pytest.raises(_lib.MVSLibraryError):
        conv2d_train.conv2d_wgrad(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), 3, 1)
    with pytest.raises(_lib.MVSLibraryError):
        conv2d_train.conv2d_dgrad(torch.zeros(1, 8, 4, 4), torch.zeros(8, 8, 3, 3), 1, 4, 4)
