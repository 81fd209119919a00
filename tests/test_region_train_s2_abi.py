"""CPU: the stride-2 backward's part of the training extension (include/train/mvs_region_train.h:
mvs_conv3d_s2_region_wgrad, its workspace size, mvs_conv3d_s2_region_dgrad): header, exports and bindings in
sync at training ABI 1, argument validation before any launch, the MVS_TRAIN_S2_BWD switch apart from
MVS_TRAIN_REGION_BWD, and the two plain functions of ops.py.  No kernel is launched."""
import ctypes
import os
import re

import pytest

from conftest import REPO

TRAIN_HEADER = os.path.join(REPO, "include", "train", "mvs_region_train.h")
S2_NAMES = ("mvs_conv3d_s2_region_wgrad_workspace_bytes", "mvs_conv3d_s2_region_wgrad", "mvs_conv3d_s2_region_dgrad")
SLOT_BYTES = 27 * 112 * 32 * 4


def _declared(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\*\s]+?\b(mvs_\w+)\s*\(", src, flags=re.M)))


def _size(*v):
    return (ctypes.c_int * 3)(*v)


def test_s2_entry_points_declared_exported_and_bound():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    names = _declared(TRAIN_HEADER)
    assert set(names) == set(_lib.TRAIN_SIGNATURES)
    for name in S2_NAMES:
        assert name in names and hasattr(lib, name), name
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1   # additions do not bump it
    assert any(os.path.basename(p) == "conv3d_s2_wgrad.hip" for p in _build.SOURCES)


def test_s2_backward_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)
    dims, pad, out = _size(8, 7, 40), _size(0, 1, 0), _size(4, 4, 20)

    def wgrad(x=fake, gy=fake, batch=2, dims=dims, pad_lo=pad, out_size=out, dw=fake, ws=fake):
        return lib.mvs_conv3d_s2_region_wgrad(x, gy, batch, dims, pad_lo, out_size, dw, ws, null)

    def dgrad(gy=fake, w27=fake, batch=2, dims=dims, pad_lo=pad, out_size=out, gx=fake):
        return lib.mvs_conv3d_s2_region_dgrad(gy, w27, batch, dims, pad_lo, out_size, gx, null)
    for call, pointers in ((wgrad, ("x", "gy", "dw", "ws")), (dgrad, ("gy", "w27", "gx"))):
        for name in pointers:
            assert call(**{name: null}) == -1, name       # null pointer
            assert call(**{name: odd}) == -1, name        # misaligned pointer
        assert call(batch=0) == -1
        assert call(dims=_size(8, 0, 40)) == -1
        assert call(pad_lo=_size(0, -1, 0)) == -1
        assert call(out_size=_size(4, 4, 0)) == -1
        assert call(dims=None) == -1
        assert call(pad_lo=None) == -1 and call(out_size=None) == -1
        assert call(dims=_size(2048, 2048, 2048)) == -3      # 2^33 voxels: past the 32-bit voxel indices
        assert call(batch=1, dims=_size(2048, 2048, 2048)) == -3
        assert call(out_size=_size(2048, 2048, 2048)) == -3

    ws = lib.mvs_conv3d_s2_region_wgrad_workspace_bytes
    for b, d, o in ((2, dims, out), (1, _size(3, 3, 3), _size(1, 1, 1)), (4, _size(192, 128, 160), _size(101, 69, 85))):
        assert ws(b, d, o) > 0 and ws(b, d, o) % SLOT_BYTES == 0   # whole [27][112][32] slots
    assert ws(0, dims, out) == 0
    assert ws(2, _size(8, 0, 40), out) == 0
    assert ws(2, dims, _size(4, 4, 0)) == 0
    assert ws(2, None, out) == 0 and ws(2, dims, None) == 0
    assert ws(1, _size(2048, 2048, 2048), out) == 0
    assert ws(1, dims, _size(2048, 2048, 2048)) == 0


@pytest.mark.parametrize("value,on", [(None, False), ("taps", False), ("", False), ("hip", True)])
def test_s2_bwd_switch(monkeypatch, value, on):
    """MVS_TRAIN_S2_BWD alone turns the stride-2 HIP backward on; s2_bwd_enabled wants an fp32 GPU tensor, so the
    switch itself is read through a stand-in with those attributes (no GPU here)."""
    import torch
    from mvs_amd import region_train

    class OnGpu:
        is_cuda, dtype = True, torch.float32
    monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    if value is None:
        monkeypatch.delenv("MVS_TRAIN_S2_BWD", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_S2_BWD", value)
    assert region_train.s2_bwd_enabled(OnGpu()) is on
    assert not region_train.s2_bwd_enabled(torch.zeros(1))            # a CPU tensor: never
    assert not region_train.bwd_enabled("s2")                         # the other switch's meaning is unchanged
    assert region_train.BWD_KINDS == ("s1",)


def test_region_bwd_switch_does_not_enable_s2(monkeypatch):
    import torch
    from mvs_amd import region_train

    class OnGpu:
        is_cuda, dtype = True, torch.float32
    monkeypatch.delenv("MVS_TRAIN_S2_BWD", raising=False)
    for v in ("hip", "s2", "s2,s1"):
        monkeypatch.setenv("MVS_TRAIN_REGION_BWD", v)
        assert not region_train.s2_bwd_enabled(OnGpu())
        assert not region_train.bwd_enabled("s2")


def test_s2_backward_ops_are_plain_functions_not_ops():
    """No new mvs:: op: the two are plain functions (like conv3d_region_wgrad) and refuse CPU tensors (no
    fallback)."""
    import torch
    from mvs_amd import _lib, ops
    assert not hasattr(torch.ops.mvs, "conv3d_s2_region_wgrad")
    assert not hasattr(torch.ops.mvs, "conv3d_s2_region_dgrad")
    with pytest.raises(_lib.MVSLibraryError):
        ops.conv3d_s2_region_wgrad(torch.zeros(1, 32, 3, 3, 3), torch.zeros(1, 1, 1, 1, 112), (0, 0, 0))
    with pytest.raises(_lib.MVSLibraryError):
        ops.conv3d_s2_region_dgrad(torch.zeros(1, 1, 1, 1, 112), torch.zeros(112, 32, 3, 3, 3), (3, 3, 3), (0, 0, 0))
