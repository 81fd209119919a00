"""GPU: deconv_1_0 (16 -> 8, the transposed region convolution whose output is the full-size volume) under autograd
on the HIP kernels (MVS_TRAIN_DECONV1=hip; mvs_amd/region_train.py _D1Box: the forward on csrc/deconv3d_region.hip
in raw mode, the weight and input gradients on csrc/deconv3d_region_bwd.hip): float64 parity of y, gx and gw with x
in NCDHW and channels-last memory, exact impulses for every tap, the weight gradient's bit-reproducibility whatever
the workspace held, three and more passes of its persistent tile loop, element offsets past 2^32 bytes, the
autograd routing, the default path unchanged, and the regulariser's whole chain.

The constants below MIRROR csrc/deconv3d_region_bwd.hip (the library does not export them):
  168   kTapRowChunks (csrc/wgrad_taprow.h), persistent workgroups (K chunks) per tap row
  16    kDwTX = kTapRowTX, coarse x-voxels of a tile
  16    kDwTR, coarse rows (flattened b, iz, iy) of a tile
  4     kDwKP, partial slots per chunk (the four waves split the tile's rows)
  tiles = ceil(Ix / 16) * ceil(B * Iz * Iy / 16);  workspace = min(tiles, 168) * 4 slots of [27][16][8]
_Plan asserts the tile count of every multi-pass case and that the library's workspace is exactly that many slots:
a change of the chunking fails there, and no case passes while running a single pass.  The input gradient has no
tile loop (one thread per input voxel, one launch over all of them): there is no multi-pass case for it.

The float64 criterion is test_region_train_s2_bwd.py's / test_region_train_t2_bwd.py's _check, unchanged: every
element within 1e-5 x the same sum over absolute values (+ 1e-30) of float64 autograd on the CPU, computed once per
shape.

Mutation run (not committed): with the accumulators zeroed at the top of the weight gradient's tile loop instead of
before it, test_d1_three_passes_match_float64 (both layouts) and test_d1_impulses_exact_past_4gb fail (3 failed, 19
passed); every other case has at most 168 tiles, one per workgroup, and cannot see it."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

CIN, COUT = 16, 8
CHUNKS, TILE_X, TILE_R, KP = 168, 16, 16, 4

# (B, x extent, crop, out_size): one input voxel; inputs whose reach starts before the box and 17+ coarse voxels
# along x; box outputs past the last input's reach, several samples; both crop parities, deeper than wide
GEOMETRIES = [(1, (1, 1, 1), (0, 0, 0), (3, 3, 3)),
              (2, (4, 5, 21), (1, 2, 5), (5, 6, 35)),
              (3, (4, 4, 20), (0, 1, 0), (8, 7, 40)),
              (1, (7, 2, 6), (2, 0, 3), (11, 4, 9))]
LAYOUTS = ["ncdhw", "channels_last"]


def _ints3(v):
    return (ctypes.c_int * 3)(*v)


def _cdiv(a, b):
    return -(-a // b)


def _tconv64(x, w, crop, out):
    """F.conv_transpose3d(x, w, stride=2), unpadded, cropped to [crop, crop + out) and zero-padded past the last
    input's reach."""
    y = F.conv_transpose3d(x, w, stride=2)
    y = y[:, :, crop[0]:crop[0] + out[0], crop[1]:crop[1] + out[1], crop[2]:crop[2] + out[2]]
    flat = []
    for have, o in reversed(list(zip(y.shape[2:], out))):   # F.pad order: W, H, D
        flat += [0, o - have]
    return F.pad(y, flat) if any(flat) else y


@functools.lru_cache(maxsize=None)
def _reference(geo, seed):
    """Inputs and the float64 CPU results (y, gx, gw), then the same sums over absolute values; computed once, the
    tests read them and leave them unchanged."""
    b, size, crop, out = geo
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, CIN, *size, generator=g)
    w = torch.randn(CIN, COUT, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, COUT, *out, generator=g)
    res = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        x64, w64 = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y64 = _tconv64(x64, w64, crop, out)
        (y64 * f(gy)).sum().backward()
        res.append((y64.detach(), x64.grad, w64.grad))
    return x, w, gy, res[0], res[1]


def _check(name, got, ref, bound):
    """The criterion; prints and returns max err / (sum over absolute values), to be read against 1e-5."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.double().cpu() - ref).abs()
    ratio = (err / (bound + 1e-30)).max().item()
    print("%s: max err %.3g, max err / bound %.3g" % (name, err.max().item(), ratio))
    assert bool((err <= 1e-5 * bound + 1e-30).all()), "%s: max err %.3g, max err / bound %.3g" % (
        name, err.max().item(), ratio)
    return ratio


def _as_cl(t):
    """A logical NCDHW tensor over channels-last memory."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def _in_layout(t, layout):
    return _as_cl(t) if layout == "channels_last" else t.contiguous()


def _is_cl(t):
    return t.permute(0, 2, 3, 4, 1).is_contiguous()


def _forward(x, w, crop, out):
    """The layer's forward as _D1Box runs it: ops.deconv3d_k3s2 in raw mode at origin 0 with pad = crop."""
    from mvs_amd import ops
    cl = ops._is_cl5(x)
    return ops.deconv3d_k3s2(x.permute(0, 2, 3, 4, 1) if cl else x, [0, 0, 0], w, list(out), list(crop), None, None,
                             None, None, channels_last=cl)


class _Plan:
    """The weight gradient's tile walk as dw_geo lays it out; asserts the library's workspace against it."""

    def __init__(self, b, size, out):
        from mvs_amd import _lib
        self.size = tuple(size)
        self.rows = b * size[0] * size[1]
        self.tiles_x = _cdiv(size[2], TILE_X)
        self.tiles = self.tiles_x * _cdiv(self.rows, TILE_R)
        self.slots = min(self.tiles, CHUNKS) * KP
        self.nbytes = _lib.load().mvs_deconv3d_k3s2_wgrad_workspace_bytes(b, CIN, COUT, _ints3(size), _ints3(out))
        assert self.nbytes == self.slots * 27 * CIN * COUT * 4, (self.nbytes, self.tiles, self.slots)

    def tile(self, b, i):
        row = (b * self.size[0] + i[0]) * self.size[1] + i[1]
        return (row // TILE_R) * self.tiles_x + i[2] // TILE_X


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_d1_forward_wgrad_and_dgrad_match_float64(geo, layout):
    """ops.deconv3d_k3s2 (raw), deconv3d_k3s2_wgrad and deconv3d_k3s2_dgrad against float64 F.conv_transpose3d
    autograd on the CPU, x in NCDHW or channels-last memory (gx comes back in the same), gy NCDHW-contiguous (read in
    place) and as a logical NCDHW view over channels-last memory (made contiguous once): the same bits."""
    from mvs_amd import ops
    b, size, crop, out = geo
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _reference(geo, 7 + sum(size))
    plan = _Plan(b, size, out)
    assert plan.slots > 0
    xg, gyg, wg = _in_layout(x.to(DEV), layout), gy.to(DEV), w.to(DEV)
    cl = layout == "channels_last" and not xg.is_contiguous()
    y = _forward(xg, wg, crop, out)
    gw = ops.deconv3d_k3s2_wgrad(xg, gyg, crop)
    gx = ops.deconv3d_k3s2_dgrad(gyg, wg, size, crop, channels_last=cl)
    assert tuple(y.shape) == (b, COUT) + out and y.is_contiguous()
    assert tuple(gx.shape) == (b, CIN) + size and (_is_cl(gx) if cl else gx.is_contiguous())
    _check("y %s %s" % (layout, geo), y, y64, ya)
    _check("gw %s %s" % (layout, geo), gw, gw64, gwa)
    _check("gx %s %s" % (layout, geo), gx, gx64, gxa)
    assert torch.equal(gw, ops.deconv3d_k3s2_wgrad(xg, _as_cl(gyg), crop))
    assert torch.equal(gx, ops.deconv3d_k3s2_dgrad(_as_cl(gyg), wg, size, crop, channels_last=cl))


# ---- exact impulses ----
IMPULSE_GEO = (2, (5, 6, 21), (1, 0, 1), (9, 13, 43))   # reach (10, 13, 42): the box ends before it along z and
                                                        # one voxel past it along x


def _impulse_voxels(geo):
    b, size, crop, out = geo
    return ((0, (0, 0, 0)), (b - 1, tuple(d - 1 for d in size)), (0, (2, 3, 10)))   # low, high corner, interior


def _taps():
    return [(t, (t // 9, (t // 3) % 3, t % 3)) for t in range(27)]


def _reached(i, crop, tap, out):
    q = tuple(2 * ii - c + tt for ii, c, tt in zip(i, crop, tap))
    return q, all(0 <= qq < o for qq, o in zip(q, out))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_d1_wgrad_tap_impulses_exact(layout):
    """One nonzero of x (1.5 at (b, ci, i)) against one of gy (-2.25 at (b, co, 2 i - crop + t)) for each of the 27
    taps, i at the low corner, the high corner of the last sample and inside: dw[ci, co, t] is exactly -3.375 and
    every other entry exactly 0 (a tap that lands outside the box has no gy to meet: all 0)."""
    from mvs_amd.ops import deconv3d_k3s2_wgrad
    B, size, crop, out = IMPULSE_GEO
    seen, off = set(), 0
    x = _in_layout(torch.zeros((B, CIN) + size, device=DEV), layout)
    gy = torch.zeros((B, COUT) + out, device=DEV)
    want = torch.zeros(CIN, COUT, 3, 3, 3, device=DEV)
    for k, (b, i) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for t, tap in _taps():
            ci, co = (7 * t + 11 * k) % CIN, (5 * t + 3 + k) % COUT
            q, inside = _reached(i, crop, tap, out)
            x[b, ci, i[0], i[1], i[2]] = 1.5
            if inside:
                gy[b, co, q[0], q[1], q[2]] = -2.25
                want[ci, co, tap[0], tap[1], tap[2]] = -3.375
                seen.add(t)
            else:
                off += 1
            dw = deconv3d_k3s2_wgrad(x, gy, crop)
            assert torch.equal(dw, want), (k, t, dw.nonzero().tolist())
            x[b, ci, i[0], i[1], i[2]] = 0.0
            if inside:
                gy[b, co, q[0], q[1], q[2]] = 0.0
                want[ci, co, tap[0], tap[1], tap[2]] = 0.0
    assert seen == set(range(27))
    assert off == (27 - 12) + (27 - 18)   # low corner: taps 0 off along z and x; high corner: tz = 2 off (z ends early)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_d1_dgrad_impulses_exact(layout):
    """gy = 1.0 at one (b, co, q), q = 2 i - crop + t for each tap of the same three voxels, with a random w:
    gx[b, :, i'] is bit-equal to w[:, co, t'] for every (i', t') that reaches q and exactly 0 elsewhere (the
    nonzero count matches: no entry of w is 0)."""
    from mvs_amd.ops import deconv3d_k3s2_dgrad
    B, size, crop, out = IMPULSE_GEO
    w = torch.randn(CIN, COUT, 3, 3, 3, generator=torch.Generator().manual_seed(3))
    assert bool((w != 0).all())
    w = w.to(DEV)
    gy = torch.zeros((B, COUT) + out, device=DEV)
    cl = layout == "channels_last"
    done = 0
    for k, (b, i) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for t, tap in _taps():
            q, inside = _reached(i, crop, tap, out)
            if not inside:
                continue
            co = (5 * t + 3 + k) % COUT
            want = torch.zeros((B, CIN) + size, device=DEV)
            hit = 0
            for _, tp in _taps():
                num = [qq + c - tt for qq, c, tt in zip(q, crop, tp)]
                if all(v % 2 == 0 and 0 <= v // 2 < d for v, d in zip(num, size)):
                    want[b, :, num[0] // 2, num[1] // 2, num[2] // 2] = w[:, co, tp[0], tp[1], tp[2]]
                    hit += 1
            assert hit >= 1
            gy[b, co, q[0], q[1], q[2]] = 1.0
            gx = deconv3d_k3s2_dgrad(gy, w, size, crop, channels_last=cl)
            gy[b, co, q[0], q[1], q[2]] = 0.0
            assert _is_cl(gx) if cl else gx.is_contiguous()
            assert torch.equal(gx, want), (k, t, (gx != want).nonzero()[:4].tolist())
            assert int(torch.count_nonzero(gx)) == hit * CIN
            done += 1
    assert done == 12 + 18 + 27


# ---- bit-reproducibility ----
def _poison_next_workspace(nbytes, value):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full((2 * nbytes // 4,), value, device=DEV)   # the next workspace comes out of this block
    torch.cuda.synchronize()
    del poison


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_d1_wgrad_reproducible_whatever_the_workspace_held(layout):
    from mvs_amd.ops import deconv3d_k3s2_wgrad
    B, size, crop, out = 2, (7, 8, 25), (1, 2, 5), (12, 14, 45)
    plan = _Plan(B, size, out)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = _in_layout(torch.randn((B, CIN) + size, device=DEV, generator=g), layout)
    gy = torch.randn((B, COUT) + out, device=DEV, generator=g)
    a = deconv3d_k3s2_wgrad(x, gy, crop)
    assert torch.equal(a, deconv3d_k3s2_wgrad(x, gy, crop))
    for value in (float("nan"), 0.0):
        _poison_next_workspace(plan.nbytes, value)
        again = deconv3d_k3s2_wgrad(x, gy, crop)
        assert bool(torch.isfinite(again).all())
        assert torch.equal(a, again)


# ---- the tile loop: every workgroup three passes and more ----
# B = 3, x (21, 45, 40): 2835 rows = 177 row tiles of 16 and one of 3, 40 voxels along x = 2 x-tiles and one of 8:
# 534 tiles = 3 x 168 + 30: every workgroup runs three tiles and 30 of them a fourth.  crop (1, 0, 1): the rows
# iz = 0 reach tz = 0 before the box (skipped rows between staged ones); the box ends one output before the reach
# along z and two along y, and goes two past it along x.
MULTI = (3, (21, 45, 40), (1, 0, 1), (41, 89, 82))
THREE_PASSES_EACH = 3 * CHUNKS


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_d1_three_passes_match_float64(layout):
    from mvs_amd import ops
    b, size, crop, out = MULTI
    plan = _Plan(b, size, out)
    assert plan.tiles == 534 and plan.tiles > THREE_PASSES_EACH and plan.tiles % CHUNKS != 0
    assert plan.rows % TILE_R != 0 and size[2] % TILE_X != 0
    assert plan.slots == CHUNKS * KP
    x, w, gy, (_, gx64, gw64), (_, gxa, gwa) = _reference(MULTI, 5)
    xg, gyg = _in_layout(x.to(DEV), layout), gy.to(DEV)
    gw = ops.deconv3d_k3s2_wgrad(xg, gyg, crop)
    gx = ops.deconv3d_k3s2_dgrad(gyg, w.to(DEV), size, crop, channels_last=layout == "channels_last")
    _check("gw %s %s" % (layout, MULTI), gw, gw64, gwa)
    _check("gx %s %s" % (layout, MULTI), gx, gx64, gxa)


# ---- element offsets past 2^32 bytes: exact impulses in zero tensors ----
GB = 1 << 30
# gy [2, 8, 160, 640, 660] = 135,168,000 voxels of 32 B = 4,325,376,000 B (2^32 + 30 MB; a sample 2.16 GB, below the
# header's 4 GB per sample); x [2, 80, 320, 330, 16] channels-last = 1.08 GB, crop 0: reach (161, 641, 661).
BIG = (2, (80, 320, 330), (0, 0, 0), (160, 640, 660))


def _need_free(peak_bytes):
    """Skip only where the device cannot hold the test: less free memory than its stated peak + 2 GB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < peak_bytes + 2 * GB:
        pytest.skip("%.1f GB free on the device; the test peaks at %.1f GB and wants 2 GB beside it"
                    % (free / GB, peak_bytes / GB))


@pytest.mark.gpu
def test_d1_impulses_exact_past_4gb():
    """gy over 4 GB: one impulse at gy's last element (byte offset past 2^32; reached only by the last input voxel
    through tap (1, 1, 1)) and one below 2^31 (o = (3, 7, 20) of sample 0, channel 1, reached by two input voxels:
    taps (1, 1, 0) and (1, 1, 2)).  gw exactly -3.375 at the one entry and 0 elsewhere; gx bit-equal to the w rows
    with its nonzeros counted over the whole output (no entry of w is 0).  A 32-bit offset reads or writes
    elsewhere.  Peak device memory 6.8 GB: gy 4.33 GB, x and gx 1.08 GB each, the workspace and the count's mask."""
    from mvs_amd.ops import deconv3d_k3s2_dgrad, deconv3d_k3s2_wgrad
    B, size, crop, out = BIG
    _need_free(int(6.8 * GB))
    plan = _Plan(B, size, out)
    assert plan.tiles > THREE_PASSES_EACH and plan.slots == CHUNKS * KP
    ovox = out[0] * out[1] * out[2]
    assert B * ovox * COUT * 4 > 1 << 32 and B * ovox < 1 << 31 and ovox * COUT * 4 < 1 << 32
    w = torch.randn(CIN, COUT, 3, 3, 3, generator=torch.Generator().manual_seed(17))
    assert bool((w != 0).all())
    w = w.to(DEV)
    last_i, last_o = tuple(d - 1 for d in size), tuple(d - 1 for d in out)
    # (b, i, tap, ci, co, input voxels that reach the output)
    cases = ((0, (1, 3, 10), (1, 1, 0), 5, 1, (((1, 3, 10), (1, 1, 0)), ((1, 3, 9), (1, 1, 2)))),
             (B - 1, last_i, (1, 1, 1), CIN - 1, COUT - 1, ((last_i, (1, 1, 1)),)))
    x = gy = gx = None
    try:
        x = torch.zeros((B,) + size + (CIN,), device=DEV).permute(0, 4, 1, 2, 3)   # channels-last memory
        gy = torch.zeros((B, COUT) + out, device=DEV)
        for k, (b, i, tap, ci, co, reach) in enumerate(cases):
            q, inside = _reached(i, crop, tap, out)
            assert inside and all(_reached(ii, crop, tt, out)[0] == q for ii, tt in reach)
            offset = ((((b * COUT + co) * out[0] + q[0]) * out[1] + q[1]) * out[2] + q[2]) * 4
            assert (offset < 1 << 31) if k == 0 else (offset == gy.numel() * 4 - 4 and offset > 1 << 32)
            x[b, ci, i[0], i[1], i[2]] = 1.5
            gy[b, co, q[0], q[1], q[2]] = -2.25
            dw = deconv3d_k3s2_wgrad(x, gy, crop)
            want = torch.zeros_like(dw)
            want[ci, co, tap[0], tap[1], tap[2]] = -3.375
            assert torch.equal(dw, want), (k, dw.nonzero().tolist())
            gy[b, co, q[0], q[1], q[2]] = 1.0
            gx = deconv3d_k3s2_dgrad(gy, w, size, crop, channels_last=True)
            for ii, tt in reach:
                assert torch.equal(gx[b, :, ii[0], ii[1], ii[2]], w[:, co, tt[0], tt[1], tt[2]]), (k, ii)
            assert int(torch.count_nonzero(gx)) == len(reach) * CIN, k
            del gx
            gx = None
            x[b, ci, i[0], i[1], i[2]] = 0.0
            gy[b, co, q[0], q[1], q[2]] = 0.0
        assert plan.tile(B - 1, last_i) == plan.tiles - 1 and q == last_o
        assert plan.tile(0, cases[0][1]) < plan.tiles - CHUNKS   # the first impulse's tile is not its chunk's last
    finally:
        del x, gy, gx
        torch.cuda.empty_cache()


# ---- routing ----
def _live_geometry(n):
    """(M, full, pad, crop) of the transposed layers at the live geometry of a volume of extent n."""
    from mvs_amd import regions
    from mvs_amd.config import pad_outpad
    pad, _ = pad_outpad(*n)
    full, M = regions.live_regions(n, pad)[:2]
    crop = tuple(lo - (2 * xlo - p) for (xlo, _), (lo, _), p in zip(M, full, pad))
    return M, full, pad, crop


D1_OPS = ("deconv3d_k3s2", "deconv3d_k3s2_wgrad", "deconv3d_k3s2_dgrad")


def _count_calls(monkeypatch, layouts=None):
    from mvs_amd import ops
    calls = []
    for name in D1_OPS:
        fn = getattr(ops, name)

        def counted(*a, _fn=fn, _name=name, **k):
            calls.append(_name)
            if layouts is not None and _name == "deconv3d_k3s2_wgrad":   # (x, gy, crop) as the backward got them
                layouts.append(("x channels-last" if ops._is_cl5(a[0]) else "x NCDHW" if a[0].is_contiguous()
                                else "x strided", "gy NCDHW" if a[1].is_contiguous() else "gy not NCDHW"))
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    return calls


ROUTE_N = (24, 20, 26)
SWITCHES = ("MVS_TRAIN_DECONV1", "MVS_TRAIN_T2_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_REGION_BWD")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_d1_box_autograd_on_the_hip_kernels(monkeypatch, layout):
    """regions._tconv_region -> region_train.d1_box at the live geometry of a (24, 20, 26) volume, B = 2, with
    MVS_TRAIN_DECONV1=hip: y, gx and gw within the float64 criterion, the forward and the two new functions called
    once each, the tap GEMMs never (they raise here); gx comes back in x's memory layout."""
    from mvs_amd import region_train, regions, tap_gemm
    for name in SWITCHES + ("MVS_TRAIN_REGION_FWD",):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("MVS_TRAIN_DECONV1", "hip")
    M, full, pad, crop = _live_geometry(ROUTE_N)
    size = tuple(regions.extent(M))
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _reference((2, size, crop, ROUTE_N), 5)
    plan = _Plan(2, size, ROUTE_N)
    print("tiles", plan.tiles)

    def refuse(*a, **k):
        raise AssertionError("a tap GEMM was called")
    monkeypatch.setattr(tap_gemm, "conv_transpose3d_box", refuse)
    monkeypatch.setattr(tap_gemm, "conv_transpose3d_backward", refuse)
    calls = _count_calls(monkeypatch)
    xg = _in_layout(x.to(DEV), layout).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    assert region_train.d1_enabled(xg) and region_train.d1_applies(xg, wg)
    assert not region_train.t2_bwd_enabled(xg) and not region_train.s2_bwd_enabled(xg)
    y = regions._tconv_region(xg, M, wg, full, pad)
    (y * gy.to(DEV)).sum().backward()
    assert sorted(calls) == sorted(D1_OPS), calls
    assert y.is_contiguous()
    assert _is_cl(xg.grad) if layout == "channels_last" else xg.grad.is_contiguous()
    _check("y", y.detach(), y64, ya)
    _check("gx", xg.grad, gx64, gxa)
    _check("gw", wg.grad, gw64, gwa)


@pytest.mark.gpu
def test_default_deconv1_path_is_the_tap_gemms(monkeypatch):
    """The switch unset: _tconv_region under autograd calls none of the three and its y, gx and gw are bit-equal to
    tap_gemm.conv_transpose3d_box's / conv_transpose3d_backward's."""
    from mvs_amd import regions, tap_gemm
    for name in SWITCHES + ("MVS_TRAIN_REGION_FWD",):
        monkeypatch.delenv(name, raising=False)
    M, full, pad, crop = _live_geometry(ROUTE_N)
    size = tuple(regions.extent(M))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, CIN, *size, generator=g).to(DEV)
    w = (torch.randn(CIN, COUT, 3, 3, 3, generator=g) * 0.05).to(DEV)
    gy = torch.randn(2, COUT, *ROUTE_N, generator=g).to(DEV)
    calls = _count_calls(monkeypatch)
    for value in (None, "taps", ""):
        if value is not None:
            monkeypatch.setenv("MVS_TRAIN_DECONV1", value)
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        y = regions._tconv_region(xg, M, wg, full, pad)
        y.backward(gy)
        assert calls == []
        with torch.enable_grad():
            y_ref = tap_gemm.conv_transpose3d_box(x, w, 2, crop, ROUTE_N)
        gx, gw = tap_gemm.conv_transpose3d_backward(x, w, 2, crop, ROUTE_N, gy)
        assert torch.equal(y.detach(), y_ref)
        assert torch.equal(xg.grad, gx) and torch.equal(wg.grad, gw)


# ---- the regulariser's chain ----
def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


CHAIN_B, CHAIN_N = 2, (16, 20, 24)   # test_regulariser_chain_with_hip_t2_backward's geometry


@functools.lru_cache(maxsize=None)
def _chain_reference():
    """The regulariser, its inputs, and the float64 / CPU fp32 forward_full gradients: computed once."""
    from weights import deterministic_state_dict
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import CostVolumeReg
    pad, outpad = pad_outpad(*CHAIN_N)
    reg = CostVolumeReg(pad=pad, outpad=outpad)
    reg.load_state_dict(deterministic_state_dict(reg.state_dict(), seed=99))
    reg.train()
    reg_c, reg_d = copy.deepcopy(reg), copy.deepcopy(reg).double()
    g = torch.Generator().manual_seed(41)
    cv = torch.rand(CHAIN_B, 32, *CHAIN_N, generator=g)
    wr = torch.randn(CHAIN_B, 1, *CHAIN_N, generator=g)
    cv_c, cv_d = cv.clone().requires_grad_(True), cv.double().requires_grad_(True)
    (reg_c.forward_full(cv_c) * wr).sum().backward()
    (reg_d.forward_full(cv_d) * wr.double()).sum().backward()
    pc = {k: v.grad for k, v in reg_c.named_parameters()}
    pd = {k: v.grad for k, v in reg_d.named_parameters()}
    return reg, cv, wr, pc, pd, cv_c.grad, cv_d.grad


@pytest.mark.gpu
@pytest.mark.parametrize("switches", [("MVS_TRAIN_DECONV1",), SWITCHES])
def test_regulariser_chain_with_hip_deconv1(monkeypatch, switches):
    """CostVolumeReg in train mode under autograd with deconv_1_0 on the HIP kernels -- alone, then with the
    transposed, stride-2 and stride-1 HIP backwards as well -- loss sum(P * Wr) on a random cost volume (B = 2,
    (16, 20, 24)): every parameter's gradient and the cost volume's, relative L2 to float64 forward_full <= 2 x the
    CPU fp32 forward_full gradient's + 1e-5 (test_regulariser_chain_with_hip_t2_backward's bound).  Prints the
    memory layouts x and gy reach the backward in."""
    from conftest import record_parity
    for name in SWITCHES + ("MVS_TRAIN_REGION_FWD",):
        monkeypatch.delenv(name, raising=False)
    for name in switches:
        monkeypatch.setenv(name, "s1" if name == "MVS_TRAIN_REGION_BWD" else "hip")
    reg, cv, wr, pc, pd, cvg_c, cvg_d = _chain_reference()
    reg_g = copy.deepcopy(reg).to(DEV)
    layouts = []
    calls = _count_calls(monkeypatch, layouts)
    cv_g = cv.to(DEV).requires_grad_(True)
    assert reg_g.live_autograd_ok(cv_g)
    (reg_g(cv_g) * wr.to(DEV)).sum().backward()
    assert sorted(calls) == sorted(D1_OPS), calls   # deconv_1_0: forward, weight gradient, input gradient, once each
    print("deconv_1_0 backward layouts:", layouts)
    pg = dict(reg_g.named_parameters())
    assert all((pg[k].grad is None) == (pd[k] is None) for k in pd)
    errs = {k: (_rel(pg[k].grad.cpu(), pd[k]), _rel(pc[k], pd[k])) for k in sorted(pd) if pd[k] is not None}
    assert {"deconv_3_0.weight", "deconv_2_0.weight", "deconv_1_0.weight"} <= set(errs)
    errs["cost_volume"] = (_rel(cv_g.grad.cpu(), cvg_d), _rel(cvg_c, cvg_d))
    record_parity("deconv1_hip_chain_grads_%d" % len(switches),
                  grad_rel_l2_gpu_vs_f64_max=max(v[0] for v in errs.values()),
                  grad_rel_l2_cpu_vs_f64_max=max(v[1] for v in errs.values()),
                  per_parameter={k: [float(a), float(b)] for k, (a, b) in errs.items()})
    worst = max(errs, key=lambda k: errs[k][0] / (2.0 * errs[k][1] + 1e-5))
    print("worst parameter %s: GPU %.3g, CPU fp32 %.3g, bound %.3g"
          % (worst, errs[worst][0], errs[worst][1], 2.0 * errs[worst][1] + 1e-5))
    for name, (e_g, e_c) in errs.items():
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
