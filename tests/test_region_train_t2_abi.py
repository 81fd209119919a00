"""CPU: the transposed layers' backward part of the training extension (include/train/mvs_region_train.h:
mvs_conv3d_t2_region_wgrad, its workspace size, mvs_conv3d_t2_region_dgrad): header, exports and bindings in
sync at training ABI 1, argument validation before any launch, the MVS_TRAIN_T2_BWD switch apart from
MVS_TRAIN_REGION_BWD and MVS_TRAIN_S2_BWD, and the two plain functions of ops.py.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TRAIN_HEADER = os.path.join(REPO, "include", "train", "mvs_region_train.h")
T2_NAMES = ("mvs_conv3d_t2_region_wgrad_workspace_bytes", "mvs_conv3d_t2_region_wgrad", "mvs_conv3d_t2_region_dgrad")
PAIRS = ((64, 32), (32, 16))
KP = {(64, 32): 1, (32, 16): 4}   # partial slots per K chunk (csrc/conv3d_t2_wgrad.hip TwTile::KP)


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\*\s]+?\b(mvs_\w+)\s*\(", src, flags=re.M)))


def _size(*v):
    return (ctypes.c_int * 3)(*v)


def test_t2_entry_points_declared_exported_and_bound():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    names = _declared(TRAIN_HEADER)
    assert set(names) == set(_lib.TRAIN_SIGNATURES)
    for name in T2_NAMES:
        assert name in names and hasattr(lib, name), name
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1   # additions do not bump it
    assert any(os.path.basename(p) == "conv3d_t2_wgrad.hip" for p in _build.SOURCES)


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_t2_backward_arguments_rejected_before_any_launch(cin, cout):
    from mvs_amd import _lib
    lib = _lib.load()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    size, crop, out = _size(4, 4, 20), _size(0, 1, 0), _size(8, 7, 40)

    def wgrad(x=fake, gy=fake, batch=2, c_in=cin, c_out=cout, in_size=size, crop=crop, out_size=out, dw=fake, ws=fake):
        return lib.mvs_conv3d_t2_region_wgrad(x, gy, batch, c_in, c_out, in_size, crop, out_size, dw, ws, null)

    def dgrad(gy=fake, w27=fake, batch=2, c_in=cin, c_out=cout, in_size=size, crop=crop, out_size=out, gx=fake):
        return lib.mvs_conv3d_t2_region_dgrad(gy, w27, batch, c_in, c_out, in_size, crop, out_size, gx, null)
    ws = lib.mvs_conv3d_t2_region_wgrad_workspace_bytes
    for call, pointers in ((wgrad, ("x", "gy", "dw", "ws")), (dgrad, ("gy", "w27", "gx"))):
        for name in pointers:
            assert call(**{name: null}) == -1, name       # null pointer
            assert call(**{name: odd}) == -1, name        # misaligned pointer
        assert call(batch=0) == -1
        assert call(in_size=_size(4, 0, 20)) == -1
        assert call(crop=_size(0, -1, 0)) == -1
        assert call(out_size=_size(8, 7, 0)) == -1
        assert call(in_size=None) == -1
        assert call(crop=None) == -1 and call(out_size=None) == -1
        for bad in ((16, 8), (32, 32), (cout, cin), (64, 16), (0, 0), (112, 32)):   # channel pairs other than the two
            assert call(c_in=bad[0], c_out=bad[1]) == -1, bad
        assert call(in_size=_size(2048, 2048, 2048)) == -3      # 2^33 voxels: past the 32-bit voxel indices
        assert call(batch=1, in_size=_size(2048, 2048, 2048)) == -3
        assert call(out_size=_size(2048, 2048, 2048)) == -3
        assert call(batch=1, out_size=_size(1024, 1024, 1024)) == -3   # 2^30 voxels, but a sample of gy >= 4 GB

    slot = 27 * cin * cout * 4 * KP[(cin, cout)]
    for b, i, o in ((2, size, out), (1, _size(1, 1, 1), _size(3, 3, 3)), (4, _size(97, 65, 81), _size(192, 128, 160))):
        assert ws(b, cin, cout, i, o) > 0 and ws(b, cin, cout, i, o) % slot == 0   # whole [27][c_in][c_out] slots
    assert ws(0, cin, cout, size, out) == 0
    assert ws(2, cin, cout, _size(4, 0, 20), out) == 0
    assert ws(2, cin, cout, size, _size(8, 7, 0)) == 0
    assert ws(2, cin, cout, None, out) == 0 and ws(2, cin, cout, size, None) == 0
    assert ws(1, cin, cout, _size(2048, 2048, 2048), out) == 0
    assert ws(1, cin, cout, size, _size(2048, 2048, 2048)) == 0
    assert ws(1, cin, cout, size, _size(1024, 1024, 1024)) == 0
    for bad in ((16, 8), (32, 32), (cout, cin), (112, 32)):
        assert ws(2, bad[0], bad[1], size, out) == 0


class _OnGpu:
    import torch as _torch
    is_cuda, dtype = True, _torch.float32


@pytest.mark.parametrize("value,on", [(None, False), ("taps", False), ("", False), ("hip", True)])
def test_t2_bwd_switch(monkeypatch, value, on):
    """MVS_TRAIN_T2_BWD alone turns the transposed layers' HIP backward on; t2_bwd_enabled wants an fp32 GPU tensor,
    so the switch itself is read through a stand-in with those attributes (no GPU here)."""
    import torch
    from mvs_amd import region_train
    monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    monkeypatch.delenv("MVS_TRAIN_S2_BWD", raising=False)
    if value is None:
        monkeypatch.delenv("MVS_TRAIN_T2_BWD", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_T2_BWD", value)
    assert region_train.t2_bwd_enabled(_OnGpu()) is on
    assert not region_train.t2_bwd_enabled(torch.zeros(1))            # a CPU tensor: never

    class Half:
        is_cuda, dtype = True, torch.float16
    assert not region_train.t2_bwd_enabled(Half())
    assert not region_train.bwd_enabled("t2")                         # the other switch's meaning is unchanged
    assert not region_train.s2_bwd_enabled(_OnGpu())
    assert region_train.BWD_KINDS == ("s1",)


def test_other_switches_do_not_enable_t2(monkeypatch):
    from mvs_amd import region_train
    monkeypatch.delenv("MVS_TRAIN_T2_BWD", raising=False)
    for v in ("hip", "t2", "s2,t2"):
        monkeypatch.setenv("MVS_TRAIN_REGION_BWD", v)
        assert not region_train.t2_bwd_enabled(_OnGpu())
        assert not region_train.bwd_enabled("t2")
    monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    monkeypatch.setenv("MVS_TRAIN_S2_BWD", "hip")
    assert not region_train.t2_bwd_enabled(_OnGpu())
    assert region_train.BWD_KINDS == ("s1",)


def test_t2_backward_ops_are_plain_functions_not_ops():
    """No new mvs:: op: the two are plain functions (like conv3d_s2_region_wgrad) and refuse CPU tensors (no
    fallback)."""
    import torch
    from mvs_amd import _lib, ops
    assert not hasattr(torch.ops.mvs, "conv3d_t2_region_wgrad")
    assert not hasattr(torch.ops.mvs, "conv3d_t2_region_dgrad")
    assert ops.T2_BWD_CHANNELS == PAIRS
    for cin, cout in PAIRS:
        with pytest.raises(_lib.MVSLibraryError):
            ops.conv3d_t2_region_wgrad(torch.zeros(1, cin, 1, 1, 1), torch.zeros(1, cout, 3, 3, 3), (0, 0, 0))
        with pytest.raises(_lib.MVSLibraryError):
            ops.conv3d_t2_region_dgrad(torch.zeros(1, cout, 3, 3, 3), torch.zeros(cin, cout, 3, 3, 3), (1, 1, 1),
                                       (0, 0, 0))
