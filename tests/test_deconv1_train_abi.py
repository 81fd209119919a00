"""CPU: deconv_1_0's backward part of the training extension (include/train/mvs_region_train.h:
mvs_deconv3d_k3s2_wgrad, its workspace size, mvs_deconv3d_k3s2_dgrad): header, exports and bindings in sync at
training ABI 1 with the main header untouched, argument validation before any launch, the MVS_TRAIN_DECONV1 switch
apart from the four other training switches, and the two plain functions of ops.py.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TRAIN_HEADER = os.path.join(REPO, "include", "train", "mvs_region_train.h")
MAIN_HEADER = os.path.join(REPO, "include", "mvs_cost_volume.h")
D1_NAMES = ("mvs_deconv3d_k3s2_wgrad_workspace_bytes", "mvs_deconv3d_k3s2_wgrad", "mvs_deconv3d_k3s2_dgrad")
CIN, COUT = 16, 8
SLOT = 27 * CIN * COUT * 4   # bytes of one [27][16][8] partial slot


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\*\s]+?\b(mvs_\w+)\s*\(", src, flags=re.M)))


def _size(*v):
    return (ctypes.c_int * 3)(*v)


def test_deconv1_entry_points_declared_exported_and_bound():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    names = _declared(TRAIN_HEADER)
    assert set(names) == set(_lib.TRAIN_SIGNATURES)
    for name in D1_NAMES:
        assert name in names and hasattr(lib, name), name
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1   # additions do not bump it
    main = _declared(MAIN_HEADER)
    assert len(main) == 45 and not set(main) & set(D1_NAMES)            # the drop-in surface is as it was
    assert set(main) == set(_lib.SIGNATURES)
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 24
    assert any(os.path.basename(p) == "deconv3d_region_bwd.hip" for p in _build.SOURCES)


def test_deconv1_backward_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    size, crop, out = _size(4, 4, 20), _size(0, 1, 0), _size(8, 7, 40)

    def wgrad(x=fake, gy=fake, flags=0, batch=2, c_in=CIN, c_out=COUT, in_size=size, crop=crop, out_size=out, dw=fake,
              ws=fake):
        return lib.mvs_deconv3d_k3s2_wgrad(x, flags, gy, batch, c_in, c_out, in_size, crop, out_size, dw, ws, null)

    def dgrad(gy=fake, w27=fake, flags=0, batch=2, c_in=CIN, c_out=COUT, in_size=size, crop=crop, out_size=out,
              gx=fake):
        return lib.mvs_deconv3d_k3s2_dgrad(gy, w27, flags, batch, c_in, c_out, in_size, crop, out_size, gx, null)
    ws = lib.mvs_deconv3d_k3s2_wgrad_workspace_bytes
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
        assert call(flags=2) == -1 and call(flags=-1) == -1           # only MVS_LAYOUT_CHANNELS_LAST is a flag
        for bad in ((8, 16), (32, 16), (64, 32), (16, 16), (8, 8), (16, 1), (0, 0), (112, 32)):
            assert call(c_in=bad[0], c_out=bad[1]) == -1, bad         # every channel pair other than (16, 8)
        assert call(in_size=_size(2048, 2048, 2048)) == -3      # 2^33 voxels: past the 32-bit voxel indices
        assert call(batch=1, in_size=_size(2048, 2048, 2048)) == -3
        assert call(out_size=_size(2048, 2048, 2048)) == -3
        assert call(batch=1, out_size=_size(1024, 1024, 1024)) == -3   # 2^30 voxels, but a sample of gy >= 4 GB
        assert call(batch=1, in_size=_size(1 << 29, 1, 1)) == -3       # 2 i - crop + t in 32 bits
        assert call(crop=_size(0, 1 << 29, 0)) == -3

    for b, i, o in ((2, size, out), (1, _size(1, 1, 1), _size(3, 3, 3)), (4, _size(97, 65, 81), _size(192, 128, 160))):
        assert ws(b, CIN, COUT, i, o) > 0 and ws(b, CIN, COUT, i, o) % SLOT == 0   # whole [27][16][8] slots
    assert ws(0, CIN, COUT, size, out) == 0
    assert ws(2, CIN, COUT, _size(4, 0, 20), out) == 0
    assert ws(2, CIN, COUT, size, _size(8, 7, 0)) == 0
    assert ws(2, CIN, COUT, None, out) == 0 and ws(2, CIN, COUT, size, None) == 0
    assert ws(1, CIN, COUT, _size(2048, 2048, 2048), out) == 0
    assert ws(1, CIN, COUT, size, _size(2048, 2048, 2048)) == 0
    assert ws(1, CIN, COUT, size, _size(1024, 1024, 1024)) == 0
    for bad in ((8, 16), (32, 16), (64, 32), (16, 16)):
        assert ws(2, bad[0], bad[1], size, out) == 0


def test_t2_entry_points_still_refuse_deconv1():
    """New entry points, not a widening of the T2 ones."""
    from mvs_amd import _lib, ops, region_train
    lib = _lib.load()
    fake, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
    size, crop, out = _size(4, 4, 20), _size(0, 1, 0), _size(8, 7, 40)
    assert lib.mvs_conv3d_t2_region_wgrad(fake, fake, 2, CIN, COUT, size, crop, out, fake, fake, null) == -1
    assert lib.mvs_conv3d_t2_region_dgrad(fake, fake, 2, CIN, COUT, size, crop, out, fake, null) == -1
    assert lib.mvs_conv3d_t2_region_wgrad_workspace_bytes(2, CIN, COUT, size, out) == 0
    assert ops.T2_BWD_CHANNELS == ((64, 32), (32, 16))
    assert region_train.T2_SHAPES == ((64, 32), (32, 16))
    assert region_train.BWD_KINDS == ("s1",)


class _OnGpu:
    import torch as _torch
    is_cuda, dtype = True, _torch.float32


OTHER_SWITCHES = ("MVS_TRAIN_REGION_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_T2_BWD", "MVS_TRAIN_REGION_FWD")


@pytest.mark.parametrize("value,on", [(None, False), ("taps", False), ("", False), ("hip", True), ("HIP", False),
                                      ("1", False), ("hip,taps", False)])
def test_deconv1_switch(monkeypatch, value, on):
    """MVS_TRAIN_DECONV1=hip alone turns the path on; d1_enabled wants an fp32 GPU tensor, so the switch itself is
    read through a stand-in with those attributes (no GPU here).  It changes none of the other switches' answers."""
    import torch
    from mvs_amd import region_train
    for name in OTHER_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if value is None:
        monkeypatch.delenv("MVS_TRAIN_DECONV1", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_DECONV1", value)
    assert region_train.d1_enabled(_OnGpu()) is on
    assert not region_train.d1_enabled(torch.zeros(1))            # a CPU tensor: never

    class Half:
        is_cuda, dtype = True, torch.float16
    assert not region_train.d1_enabled(Half())
    assert not region_train.d1_applies(torch.zeros(1), torch.zeros(16, 8, 3, 3, 3))
    assert not region_train.bwd_enabled("s1") and not region_train.bwd_enabled("t2")
    assert not region_train.bwd_enabled("d1")
    assert not region_train.s2_bwd_enabled(_OnGpu())
    assert not region_train.t2_bwd_enabled(_OnGpu())
    assert region_train.BWD_KINDS == ("s1",)
    assert region_train.T2_SHAPES == ((64, 32), (32, 16))


def test_other_switches_do_not_enable_deconv1(monkeypatch):
    from mvs_amd import region_train
    monkeypatch.delenv("MVS_TRAIN_DECONV1", raising=False)
    for name in OTHER_SWITCHES:
        for v in ("hip", "taps", "s1", "t2", "s1,t2", "s2,t2", "d1", "deconv1"):
            monkeypatch.setenv(name, v)
            assert not region_train.d1_enabled(_OnGpu()), (name, v)
        monkeypatch.delenv(name, raising=False)
    for name in OTHER_SWITCHES:       # all four on at once
        monkeypatch.setenv(name, "hip")
    assert not region_train.d1_enabled(_OnGpu())
    assert region_train.BWD_KINDS == ("s1",)
    assert region_train.T2_SHAPES == ((64, 32), (32, 16))


def test_deconv1_d1_applies_wants_the_16_8_weight(monkeypatch):
    """d1_applies through the stand-in: only the (16, 8, 3, 3, 3) weight, only with the switch on."""
    import torch
    from mvs_amd import region_train
    monkeypatch.setenv("MVS_TRAIN_DECONV1", "hip")
    assert region_train.d1_applies(_OnGpu(), torch.zeros(16, 8, 3, 3, 3))
    for shape in ((32, 16, 3, 3, 3), (64, 32, 3, 3, 3), (8, 16, 3, 3, 3), (16, 8, 1, 3, 3)):
        assert not region_train.d1_applies(_OnGpu(), torch.zeros(*shape)), shape
    with torch.no_grad():
        assert not region_train.d1_applies(_OnGpu(), torch.zeros(16, 8, 3, 3, 3))
    monkeypatch.delenv("MVS_TRAIN_DECONV1")
    assert not region_train.d1_applies(_OnGpu(), torch.zeros(16, 8, 3, 3, 3))


def test_deconv1_backward_ops_are_plain_functions_not_ops():
    """No new mvs:: op: the two are plain functions (like conv3d_t2_region_wgrad) and refuse CPU tensors (no
    fallback)."""
    import torch
    from mvs_amd import _lib, ops
    assert not hasattr(torch.ops.mvs, "deconv3d_k3s2_wgrad")
    assert not hasattr(torch.ops.mvs, "deconv3d_k3s2_dgrad")
    assert ops.DECONV1_CHANNELS == (CIN, COUT)
    with pytest.raises(_lib.MVSLibraryError):
        ops.deconv3d_k3s2_wgrad(torch.zeros(1, CIN, 1, 1, 1), torch.zeros(1, COUT, 3, 3, 3), (0, 0, 0))
    with pytest.raises(_lib.MVSLibraryError):
        ops.deconv3d_k3s2_dgrad(torch.zeros(1, COUT, 3, 3, 3), torch.zeros(CIN, COUT, 3, 3, 3), (1, 1, 1), (0, 0, 0))
