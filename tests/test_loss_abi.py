"""CPU: the objective in the training extension of the C ABI (include/train/mvs_loss.h: mvs_masked_mae_plan /
_workspace_bytes / _fwd / _bwd) -- header, exports and bindings in sync, every refusal before any launch (dimensions
and fake pointers only: no memory is touched), the plan and workspace queries against the formula mirrored here -- and
mvs_amd.loss on CPU tensors, where it is the reference's torch expression.  No kernel is launched."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO

LOSS_HEADER = os.path.join(REPO, "include", "train", "mvs_loss.h")
NAMES = ("mvs_masked_mae_plan", "mvs_masked_mae_workspace_bytes", "mvs_masked_mae_fwd", "mvs_masked_mae_bwd")
NULL, FAKE, ODD = ctypes.c_void_p(0), ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1002)
C_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def _plan(batch, n):
    """The plan mirrored: four-element items, 256 of them per workgroup and pass, about 1024 workgroups over the
    batch, none without a first item."""
    items = -(-n // 4)
    wg = max(1, min(-(-items // 256), -(-1024 // batch)))
    return wg, -(-items // (wg * 256))


def _header_signatures():
    """name -> (restype, argtypes) read from the header's declarations: pointers are void*, the rest by name."""
    src = re.sub(r"/\*.*?\*/", "", open(LOSS_HEADER).read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^\s*(int|size_t)\s+(mvs_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (C_TYPES[res], types)
    return out


def test_package_exports_the_loss():
    import mvs_amd
    from mvs_amd.loss import depth_accuracy, loss_fcn
    assert mvs_amd.loss_fcn is loss_fcn and mvs_amd.depth_accuracy is depth_accuracy
    from mvs_amd import config
    assert config.ACC_THRESH == 0.05
    # two ops, in the training namespace; the drop-in namespace gains none
    assert hasattr(torch.ops.mvs_train, "masked_mae") and hasattr(torch.ops.mvs_train, "masked_mae_bwd")
    assert not hasattr(torch.ops.mvs, "masked_mae") and not hasattr(torch.ops.mvs, "masked_mae_bwd")


def test_header_exports_and_bindings():
    from mvs_amd import _build, _lib
    lib = _lib.load()
    declared = _header_signatures()
    assert sorted(declared) == sorted(NAMES) == sorted(_lib.LOSS_SIGNATURES)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name not in _lib.SIGNATURES and name not in _lib.TRAIN_SIGNATURES
        res, args = _lib.LOSS_SIGNATURES[name]
        assert (res, list(args)) == declared[name], name
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == list(args)
    assert lib.mvs_train_abi_version() == _lib.TRAIN_ABI_VERSION == 1    # additive: not bumped
    assert LOSS_HEADER in [os.path.abspath(p) for p in _build.HEADERS]
    assert any(os.path.basename(p) == "loss.hip" for p in _build.SOURCES)
    assert "loss.hip" not in _build.SOURCE_FLAGS    # default build flags


def test_plan_and_workspace_queries():
    from mvs_amd import _lib, loss
    lib = _lib.load()
    for batch in (1, 2, 3, 4, 7, 1024, 1025, 65535):
        for h, w in ((1, 1), (1, 3), (2, 3), (5, 7), (9, 33), (17, 40), (128, 160), (1, 1025), (1000, 1000),
                     (32768, 65535)):
            wg, passes = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.mvs_masked_mae_plan(batch, h, w, ctypes.byref(wg), ctypes.byref(passes)) == 0
            assert (wg.value, passes.value) == _plan(batch, h * w), (batch, h, w)
            assert lib.mvs_masked_mae_workspace_bytes(batch, h, w) == wg.value * batch * 5 * 8
            assert loss.plan(batch, h, w) == (wg.value, passes.value)
    assert lib.mvs_masked_mae_plan(4, 128, 160, None, None) == 0    # null outputs are allowed
    assert _plan(4, 128 * 160) == (20, 1) and _plan(3, 10 ** 6) == (342, 3)    # the cfg-2 maps; a multi-pass walk


def test_arguments_rejected_before_any_launch():
    from mvs_amd import _lib, loss
    lib = _lib.load()

    def fwd(gt=FAKE, x0=FAKE, x1=FAKE, batch=2, h=5, w=7, thresh=0.05, l0=FAKE, l1=FAKE, a0=FAKE, a1=FAKE, nv=FAKE,
            ws=FAKE):
        return lib.mvs_masked_mae_fwd(gt, x0, x1, batch, h, w, thresh, l0, l1, a0, a1, nv, ws, NULL)

    def bwd(gt=FAKE, x0=FAKE, x1=FAKE, c0=FAKE, c1=FAKE, batch=2, h=5, w=7, g0=FAKE, g1=FAKE):
        return lib.mvs_masked_mae_bwd(gt, x0, x1, c0, c1, batch, h, w, g0, g1, NULL)

    def queries(batch, h, w):
        wg = ctypes.c_int(-7)
        st = lib.mvs_masked_mae_plan(batch, h, w, ctypes.byref(wg), None)
        assert st == 0 or wg.value == -7          # a refused plan writes nothing
        return st, lib.mvs_masked_mae_workspace_bytes(batch, h, w)

    for name in ("gt", "x0", "x1", "l0", "l1", "a0", "a1", "nv", "ws"):
        assert fwd(**{name: NULL}) == -1 and fwd(**{name: ODD}) == -1, name
    assert fwd(ws=ctypes.c_void_p(0x1004)) == -1    # the slots are 8-byte words
    for name in ("gt", "x0", "x1", "c0", "c1", "g0", "g1"):
        assert bwd(**{name: NULL}) == -1 and bwd(**{name: ODD}) == -1, name
    for thresh in (-1e-3, -float("inf"), float("nan")):
        assert fwd(thresh=thresh) == -1, thresh
    for kw in ({"batch": 0}, {"batch": -1}, {"h": 0}, {"w": 0}, {"h": -4, "w": -4}):
        assert fwd(**kw) == -1 and bwd(**kw) == -1, kw
        assert queries(kw.get("batch", 2), kw.get("h", 5), kw.get("w", 7)) == (-1, 0)
    # a per-sample element count at or past 2^31; a batch past grid.y
    for batch, h, w in ((1, 32768, 65536), (2, 65536, 65536), (1, 2 ** 31 - 1, 2), (65536, 5, 7)):
        assert fwd(batch=batch, h=h, w=w) == -3 and bwd(batch=batch, h=h, w=w) == -3, (batch, h, w)
        assert queries(batch, h, w) == (-3, 0)
        with pytest.raises(ValueError):
            loss.plan(batch, h, w)
    assert queries(1, 32768, 65535)[0] == 0 and queries(65535, 5, 7)[0] == 0    # just below: dimensions accepted
    # the ops themselves have no CPU kernel (loss_fcn, not the op, holds the torch expression)
    z = torch.zeros(1, 1, 2, 2)
    with pytest.raises(_lib.MVSLibraryError):
        loss.masked_mae(z, z, z, 0.05)
    with pytest.raises(_lib.MVSLibraryError):
        loss.masked_mae_bwd(z, z, z, torch.zeros(1), torch.zeros(1))
    with pytest.raises(ValueError):
        loss.depth_accuracy(z, z, z, thresh=-0.5)


def _cpu_maps(dtype, seed=11, shape=(3, 1, 9, 13)):
    g = torch.Generator().manual_seed(seed)
    gt = (400.0 + 300.0 * torch.randn(shape, generator=g)).to(dtype)
    gt[torch.rand(shape, generator=g) < 0.3] = 0.0
    gt[1, 0, :, :] = 0.0
    gt[1, 0, -1, 2] = -3.5                                   # a sample with one valid pixel, a negative depth
    initial = (gt + 5.0 * torch.randn(shape, generator=g).to(dtype))
    refined = (gt + 2.0 * torch.randn(shape, generator=g).to(dtype))
    initial[0, 0, 0, :4] = gt[0, 0, 0, :4]                   # exact ties
    return gt, initial, refined


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_tensors_take_the_reference_expression(dtype):
    import mvs_oracle
    from mvs_amd.loss import loss_fcn
    gt, initial, refined = _cpu_maps(dtype)
    leaves = [[t.clone().requires_grad_(True) for t in (initial, refined)] for _ in range(2)]
    got = loss_fcn(gt, *leaves[0])
    want = mvs_oracle.loss_fcn(gt, *leaves[1])
    for a, b in zip(got, want):
        assert a.dim() == 0 and a.dtype == dtype and torch.equal(a, b)
    got[0].backward()
    want[0].backward()
    for a, b in zip(*leaves):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    # other shapes too: the reference expression wants any 4-D maps
    gt, initial, refined = _cpu_maps(dtype, seed=5, shape=(2, 3, 4, 5))
    for a, b in zip(loss_fcn(gt, initial, refined), mvs_oracle.loss_fcn(gt, initial, refined)):
        assert torch.equal(a, b)


def test_depth_accuracy_on_cpu_tensors():
    from mvs_amd.loss import depth_accuracy
    gt = torch.tensor([[[[8.0, 0.0, -4.0, 2.0]]], [[[0.0, 16.0, 16.0, 0.0]]]])
    # 0.25 |gt| = 2, -, 1, 0.5 and -, 4, 4, -
    initial = torch.tensor([[[[10.0, 5.0, -5.0, 2.75]]], [[[1.0, 12.0, 11.5, 0.0]]]])
    refined = gt.clone().requires_grad_(True)
    a0, a1 = depth_accuracy(gt, initial, refined, thresh=0.25)
    assert a0.dim() == 0 and not a0.requires_grad and not a1.requires_grad
    want = (torch.tensor([2.0, 1.0]) / torch.tensor([3.0, 2.0])).mean()
    assert torch.equal(a0, want) and a1.item() == 1.0    # on the boundary counts as accurate
    a0, _ = depth_accuracy(gt.double(), initial.double(), refined.detach().double())
    assert a0.dtype == torch.float64 and a0.item() == 0.0
