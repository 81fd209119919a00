"""CPU: the training extension of the C ABI (include/train/mvs_region_train.h, _lib.TRAIN_SIGNATURES):
header, exports and bindings in sync, versioned apart from the drop-in ABI (whose three pins of
tests/test_library.py are re-asserted here), argument validation before any launch, and the
MVS_TRAIN_REGION_BWD switch.  No kernel is launched."""
import ctypes
import glob
import os
import re

import pytest

from conftest import REPO

TRAIN_HEADER = os.path.join(REPO, "include", "train", "mvs_region_train.h")


def _declared(paths):
    names = []
    for h in paths:
        src = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names += re.findall(r"^\s*(?:const\s+)?[\w\*\s]+?\b(mvs_\w+)\s*\(", src, flags=re.M)
    return sorted(set(names))


def test_train_header_exports_and_bindings_in_sync():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    names = _declared([TRAIN_HEADER])
    assert "mvs_conv3d_region_wgrad" in names and "mvs_conv3d_region_wgrad_workspace_bytes" in names
    for name in names:
        assert hasattr(lib, name), name
    assert set(names) == set(_lib.TRAIN_SIGNATURES)
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1
    assert "#define MVS_TRAIN_ABI_VERSION 1" in open(TRAIN_HEADER).read()
    assert TRAIN_HEADER in [os.path.abspath(p) for p in _build.HEADERS]
    assert any(os.path.basename(p) == "conv3d_region_wgrad.hip" for p in _build.SOURCES)


def test_drop_in_abi_pins_unchanged():
    """tests/test_library.py's pins: 45 declarations in include/*.h, the same 45 bound, ABI 24; the training
    functions are in neither."""
    from mvs_amd import _lib
    lib = _lib.load()
    names = _declared(glob.glob(os.path.join(REPO, "include", "*.h")))
    assert len(names) == 45, names
    assert set(names) == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 45
    assert lib.mvs_abi_version() == _lib.ABI_VERSION == 24
    assert not set(_lib.TRAIN_SIGNATURES) & set(_lib.SIGNATURES)


def test_region_wgrad_arguments_rejected_before_any_launch():
    from mvs_amd import _lib
    lib = _lib.load()
    null, fake, odd = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1004)

    def size(*v):
        return (ctypes.c_int * 3)(*v)
    ok = size(5, 6, 7)

    def call(x=fake, gy=fake, batch=2, channels=32, in_size=ok, dw=fake, ws=fake):
        return lib.mvs_conv3d_region_wgrad(x, gy, batch, channels, in_size, dw, ws, null)
    for name in ("x", "gy", "dw", "ws"):
        assert call(**{name: null}) == -1, name       # null pointer
        assert call(**{name: odd}) == -1, name        # misaligned pointer
    assert call(in_size=None) == -1
    assert call(batch=0) == -1
    assert call(channels=24) == -1
    assert call(channels=8) == -1 and call(channels=128) == -1
    assert call(in_size=size(2, 5, 5)) == -1
    assert call(in_size=size(5, 5, 2)) == -1
    assert call(in_size=size(2048, 2048, 2048)) == -3    # 2^33 voxels: past the 32-bit row / tile indices
    assert call(batch=4, in_size=size(1024, 1024, 512)) == -3
    for c in (16, 32, 64):
        assert lib.mvs_conv3d_region_wgrad_workspace_bytes(2, c, ok) > 0
        assert lib.mvs_conv3d_region_wgrad_workspace_bytes(2, c, ok) % (27 * c * c * 4) == 0   # whole [27][C][C] slots
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(1, 16, size(3, 3, 3)) > 0
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(2, 24, ok) == 0
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(0, 32, ok) == 0
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(2, 32, size(2, 5, 5)) == 0
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(2, 32, None) == 0
    assert lib.mvs_conv3d_region_wgrad_workspace_bytes(1, 32, size(2048, 2048, 2048)) == 0


@pytest.mark.parametrize("value,s1_on", [(None, False), ("taps", False), ("s1", True), ("hip", True),
                                         ("s2,t2", False), ("s2,s1", True), ("", False)])
def test_region_bwd_switch(monkeypatch, value, s1_on):
    from mvs_amd import region_train
    if value is None:
        monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    else:
        monkeypatch.setenv("MVS_TRAIN_REGION_BWD", value)
    assert region_train.bwd_enabled("s1") is s1_on
    # kinds without a HIP backward stay on the tap GEMMs whatever the switch names
    assert not region_train.bwd_enabled("s2") and not region_train.bwd_enabled("t2")
    for c in region_train.S1_CHANNELS:
        assert region_train.bwd_enabled("s1", c) is (s1_on and c in region_train.S1_BWD_CHANNELS)
    assert not region_train.bwd_enabled("s1", 24)


def test_region_wgrad_is_a_plain_function_not_an_op():
    """No new mvs:: op: ops.conv3d_region_wgrad is a plain function (like conv3d_k3_wgrad) and refuses a CPU
    tensor (no fallback)."""
    import torch
    from mvs_amd import _lib, ops
    assert not hasattr(torch.ops.mvs, "conv3d_region_wgrad")
    with pytest.raises(_lib.MVSLibraryError):
        ops.conv3d_region_wgrad(torch.zeros(1, 3, 3, 3, 16), torch.zeros(1, 1, 1, 1, 16))
