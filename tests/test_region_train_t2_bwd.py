"""GPU: the transposed region convolutions' HIP backward (MVS_TRAIN_T2_BWD=hip; mvs_amd/region_train.py _T2Box:
the weight gradient on csrc/conv3d_t2_wgrad.hip, the input gradient on the region kernel's stride-2 mode with the
channels-last output gradient as the volume, three partial sums per output) for deconv_3_0 (64 -> 32) and
deconv_2_0 (32 -> 16): float64 parity, exact impulses for every tap, the weight gradient's bit-reproducibility
whatever the workspace held, three and more passes of its persistent tile loop, element offsets past 2^32 bytes,
the autograd routing, the default path unchanged, and the regulariser's whole chain.

The constants below MIRROR csrc/conv3d_t2_wgrad.hip (the library does not export them):
  168      kTapRowChunks (csrc/wgrad_taprow.h), persistent workgroups (K chunks) per tap row
  16       kTapRowTX, coarse x-voxels of a tile
  6 / 12   TwTile::TR, coarse rows (flattened b, iz, iy) of a tile for (64, 32) / (32, 16)
  1 / 4    TwTile::KP, partial slots per chunk ((32, 16): the four waves split the tile's rows)
  tiles = ceil(Ix / 16) * ceil(B * Iz * Iy / TR);  workspace = min(tiles, 168) * KP slots of [27][c_in][c_out]
_plan asserts the tile count of every multi-pass case and that the library's workspace is exactly that many
slots: a change of the chunking fails there, and no case passes while running a single pass.

The float64 criterion is test_region_train_s2_bwd.py's _check, unchanged: every element within 1e-5 x the same
sum over absolute values (+ 1e-30) of float64 autograd on the CPU, computed once per shape.

Mutation run (not committed): with the accumulators zeroed at the top of the tile loop instead of before it,
test_t2_three_passes_match_float64 (both pairs) and test_t2_impulses_exact_past_4gb fail (3 failed, 20 passed);
every other case has at most 168 tiles, one per workgroup, and cannot see it."""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

PAIRS = [(64, 32), (32, 16)]
CHUNKS, TILE_X = 168, 16
TR = {(64, 32): 6, (32, 16): 12}
KP = {(64, 32): 1, (32, 16): 4}

# (B, x extent, crop, out_size): one input voxel; inputs whose reach starts before the box and 17+ coarse voxels
# along x; box outputs past the last input's reach, several samples; both crop parities, deeper than wide
GEOMETRIES = [(1, (1, 1, 1), (0, 0, 0), (3, 3, 3)),
              (2, (4, 5, 21), (1, 2, 5), (5, 6, 35)),
              (3, (4, 4, 20), (0, 1, 0), (8, 7, 40)),
              (1, (7, 2, 6), (2, 0, 3), (11, 4, 9))]


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
def _reference(pair, geo, seed):
    """Inputs and the float64 CPU results (y, gx, gw), then the same sums over absolute values; computed once, the
    tests read them and leave them unchanged."""
    (cin, cout), (b, size, crop, out) = pair, geo
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, cin, *size, generator=g)
    w = torch.randn(cin, cout, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, cout, *out, generator=g)
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
    """A logical NCDHW tensor over channels-last memory (what autograd hands _T2Box.backward at training shapes)."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


class _Plan:
    """The weight gradient's tile walk as tw_geo lays it out; asserts the library's workspace against it."""

    def __init__(self, pair, b, size, out):
        from mvs_amd import _lib
        self.pair, self.size, self.tr = pair, tuple(size), TR[pair]
        self.rows = b * size[0] * size[1]
        self.tiles_x = _cdiv(size[2], TILE_X)
        self.tiles = self.tiles_x * _cdiv(self.rows, self.tr)
        self.slots = min(self.tiles, CHUNKS) * KP[pair]
        self.nbytes = _lib.load().mvs_conv3d_t2_region_wgrad_workspace_bytes(b, pair[0], pair[1], _ints3(size),
                                                                            _ints3(out))
        assert self.nbytes == self.slots * 27 * pair[0] * pair[1] * 4, (self.nbytes, self.tiles, self.slots)

    def tile(self, b, i):
        row = (b * self.size[0] + i[0]) * self.size[1] + i[1]
        return (row // self.tr) * self.tiles_x + i[2] // TILE_X


@pytest.mark.gpu
@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_wgrad_and_dgrad_match_float64(pair, geo):
    """ops.conv3d_t2_region_wgrad and conv3d_t2_region_dgrad against float64 F.conv_transpose3d autograd on the
    CPU, gy NCDHW-contiguous (copied inside) and over channels-last memory (read in place): the same bits."""
    from mvs_amd import ops
    b, size, crop, out = geo
    x, w, gy, (_, gx64, gw64), (_, gxa, gwa) = _reference(pair, geo, 7 + sum(size) + pair[0])
    plan = _Plan(pair, b, size, out)
    assert plan.slots > 0
    xg, gyg = x.to(DEV), gy.to(DEV)
    gw = ops.conv3d_t2_region_wgrad(xg, gyg, crop)
    gx = ops.conv3d_t2_region_dgrad(gyg, w.to(DEV), size, crop)
    assert tuple(gx.shape) == (b, pair[0]) + size and gx.permute(0, 2, 3, 4, 1).is_contiguous()
    _check("gw %s %s" % (pair, geo), gw, gw64, gwa)
    _check("gx %s %s" % (pair, geo), gx, gx64, gxa)
    assert torch.equal(gw, ops.conv3d_t2_region_wgrad(_as_cl(xg), _as_cl(gyg), crop))
    assert torch.equal(gx, ops.conv3d_t2_region_dgrad(_as_cl(gyg), w.to(DEV), size, crop))


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
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_wgrad_tap_impulses_exact(pair):
    """One nonzero of x (-2.25 at (b, ci, i)) against one of gy (1.5 at (b, co, 2 i - crop + t)) for each of the 27
    taps, i at the low corner, the high corner of the last sample and inside: dw[ci, co, t] is exactly -3.375 and
    every other entry exactly 0 (a tap that lands outside the box has no gy to meet: all 0)."""
    from mvs_amd.ops import conv3d_t2_region_wgrad
    cin, cout = pair
    B, size, crop, out = IMPULSE_GEO
    seen, off = set(), 0
    x = torch.zeros((B,) + size + (cin,), device=DEV).permute(0, 4, 1, 2, 3)
    gy = torch.zeros((B,) + out + (cout,), device=DEV).permute(0, 4, 1, 2, 3)
    want = torch.zeros(cin, cout, 3, 3, 3, device=DEV)
    for k, (b, i) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for t, tap in _taps():
            ci, co = (7 * t + 11 * k) % cin, (5 * t + 3 + k) % cout
            q, inside = _reached(i, crop, tap, out)
            x[b, ci, i[0], i[1], i[2]] = -2.25
            if inside:
                gy[b, co, q[0], q[1], q[2]] = 1.5
                want[ci, co, tap[0], tap[1], tap[2]] = -3.375
                seen.add(t)
            else:
                off += 1
            dw = conv3d_t2_region_wgrad(x, gy, crop)
            assert torch.equal(dw, want), (k, t, dw.nonzero().tolist())
            x[b, ci, i[0], i[1], i[2]] = 0.0
            if inside:
                gy[b, co, q[0], q[1], q[2]] = 0.0
                want[ci, co, tap[0], tap[1], tap[2]] = 0.0
    assert seen == set(range(27))
    assert off == (27 - 12) + (27 - 18)   # low corner: taps 0 off along z and x; high corner: tz = 2 off (z ends early)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_dgrad_impulses_exact(pair):
    """gy = 1.0 at one (b, co, q), q = 2 i - crop + t for each tap of the same three voxels, with a random w:
    gx[b, :, i'] is bit-equal to w[:, co, t'] for every (i', t') that reaches q and exactly 0 elsewhere."""
    from mvs_amd.ops import conv3d_t2_region_dgrad
    cin, cout = pair
    B, size, crop, out = IMPULSE_GEO
    w = torch.randn(cin, cout, 3, 3, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    gy = torch.zeros((B,) + out + (cout,), device=DEV).permute(0, 4, 1, 2, 3)
    done = 0
    for k, (b, i) in enumerate(_impulse_voxels(IMPULSE_GEO)):
        for t, tap in _taps():
            q, inside = _reached(i, crop, tap, out)
            if not inside:
                continue
            co = (5 * t + 3 + k) % cout
            want = torch.zeros((B, cin) + size, device=DEV)
            hit = 0
            for _, tp in _taps():
                num = [qq + c - tt for qq, c, tt in zip(q, crop, tp)]
                if all(v % 2 == 0 and 0 <= v // 2 < d for v, d in zip(num, size)):
                    want[b, :, num[0] // 2, num[1] // 2, num[2] // 2] = w[:, co, tp[0], tp[1], tp[2]]
                    hit += 1
            assert hit >= 1
            gy[b, co, q[0], q[1], q[2]] = 1.0
            gx = conv3d_t2_region_dgrad(gy, w, size, crop)
            gy[b, co, q[0], q[1], q[2]] = 0.0
            assert torch.equal(gx, want), (k, t, (gx != want).nonzero()[:4].tolist())
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
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_wgrad_reproducible_whatever_the_workspace_held(pair):
    from mvs_amd.ops import conv3d_t2_region_wgrad
    cin, cout = pair
    B, size, crop, out = 2, (7, 8, 25), (1, 2, 5), (12, 14, 45)
    plan = _Plan(pair, B, size, out)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((B, cin) + size, device=DEV, generator=g)
    gy = torch.randn((B, cout) + out, device=DEV, generator=g)
    a = conv3d_t2_region_wgrad(x, gy, crop)
    assert torch.equal(a, conv3d_t2_region_wgrad(x, gy, crop))
    for value in (float("nan"), 0.0):
        _poison_next_workspace(plan.nbytes, value)
        again = conv3d_t2_region_wgrad(x, gy, crop)
        assert bool(torch.isfinite(again).all())
        assert torch.equal(a, again)


# ---- the tile loop: three passes and more ----
# (64, 32): B = 3, x (16, 15, 40): 720 rows = 120 row tiles of 6, 40 voxels along x = 2 x-tiles and one of 8: 360
# tiles.  (32, 16): B = 3, x (24, 20, 40): 1440 rows = 120 row tiles of 12, 3 x-tiles: 360.  360 = 2 x 168 + 24:
# every workgroup runs two tiles and 24 of them a third.  crop (1, 0, 1): the rows iz = 0 reach tz = 0 before the
# box (skipped rows between staged ones); the box ends one output before the reach along z and goes two past it
# along x.
MULTI = {(64, 32): (3, (16, 15, 40), (1, 0, 1), (31, 31, 82)),
         (32, 16): (3, (24, 20, 40), (1, 0, 1), (47, 41, 82))}
THREE_PASSES = 2 * CHUNKS + 1


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_three_passes_match_float64(pair):
    from mvs_amd import ops
    b, size, crop, out = MULTI[pair]
    plan = _Plan(pair, b, size, out)
    assert plan.tiles == 360 and plan.tiles >= THREE_PASSES and plan.tiles % CHUNKS != 0
    assert plan.slots == CHUNKS * KP[pair]
    x, w, gy, (_, gx64, gw64), (_, gxa, gwa) = _reference(pair, MULTI[pair], 5)
    gyg = _as_cl(gy.to(DEV))
    gw = ops.conv3d_t2_region_wgrad(_as_cl(x.to(DEV)), gyg, crop)
    gx = ops.conv3d_t2_region_dgrad(gyg, w.to(DEV), size, crop)
    _check("gw %s %s" % (pair, MULTI[pair]), gw, gw64, gwa)
    _check("gx %s %s" % (pair, MULTI[pair]), gx, gx64, gxa)


# ---- element offsets past 2^32 bytes: exact impulses in zero tensors ----
GB = 1 << 30
# gy [2, 65, 512, 1024, 16] = 68,157,440 voxels of 64 B = 4,362,076,160 B (2^32 + 67 MB; a sample 2.18 GB, below
# the input gradient's 4 GB descriptor); x [2, 32, 256, 512, 32] = 1.07 GB, crop 0: reach (65, 513, 1025).
BIG = (2, (32, 256, 512), (0, 0, 0), (65, 512, 1024))


def _need_free(peak_bytes):
    """Skip only where the device cannot hold the test: less free memory than its stated peak + 2 GB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < peak_bytes + 2 * GB:
        pytest.skip("%.1f GB free on the device; the test peaks at %.1f GB and wants 2 GB beside it"
                    % (free / GB, peak_bytes / GB))


@pytest.mark.gpu
def test_t2_impulses_exact_past_4gb():
    """(32, 16) with gy over 4 GB: one impulse at gy's last element (byte offset past 2^32; reached only by the
    last input voxel through tap (2, 1, 1)) and one below 2^31 (o = (3, 7, 20) of sample 0, reached by two input
    voxels: taps (1, 1, 0) and (1, 1, 2)).  gw exactly -3.375 at the one entry and 0 elsewhere; gx bit-equal to the
    w rows with its nonzeros counted over the whole output (no entry of w is 0).  A 32-bit offset reads or writes
    elsewhere.  Peak device memory 6.8 GB: gy 4.36 GB, x and gx 1.07 GB each, the workspace and the count's mask."""
    from mvs_amd.ops import conv3d_t2_region_dgrad, conv3d_t2_region_wgrad
    pair = cin, cout = (32, 16)
    B, size, crop, out = BIG
    _need_free(int(6.8 * GB))
    plan = _Plan(pair, B, size, out)
    assert plan.tiles >= THREE_PASSES and plan.slots == CHUNKS * KP[pair]
    assert B * out[0] * out[1] * out[2] * cout * 4 > 1 << 32 and B * out[0] * out[1] * out[2] < 1 << 31
    w = torch.randn(cin, cout, 3, 3, 3, generator=torch.Generator().manual_seed(17))
    assert bool((w != 0).all())
    w = w.to(DEV)
    last_i, last_o = tuple(d - 1 for d in size), tuple(d - 1 for d in out)
    # (b, i, tap, ci, co, input voxels that reach the output)
    cases = ((0, (1, 3, 10), (1, 1, 0), 5, 9, (((1, 3, 10), (1, 1, 0)), ((1, 3, 9), (1, 1, 2)))),
             (B - 1, last_i, (2, 1, 1), cin - 1, cout - 1, ((last_i, (2, 1, 1)),)))
    x = gy = gx = None
    try:
        x = torch.zeros((B,) + size + (cin,), device=DEV).permute(0, 4, 1, 2, 3)
        gy = torch.zeros((B,) + out + (cout,), device=DEV).permute(0, 4, 1, 2, 3)
        for k, (b, i, tap, ci, co, reach) in enumerate(cases):
            q, inside = _reached(i, crop, tap, out)
            assert inside and all(_reached(ii, crop, tt, out)[0] == q for ii, tt in reach)
            offset = ((((b * out[0] + q[0]) * out[1] + q[1]) * out[2] + q[2]) * cout + co) * 4
            assert (offset < 1 << 31) if k == 0 else (offset == gy.numel() * 4 - 4 and offset > 1 << 32)
            x[b, ci, i[0], i[1], i[2]] = -2.25
            gy[b, co, q[0], q[1], q[2]] = 1.5
            dw = conv3d_t2_region_wgrad(x, gy, crop)
            want = torch.zeros_like(dw)
            want[ci, co, tap[0], tap[1], tap[2]] = -3.375
            assert torch.equal(dw, want), (k, dw.nonzero().tolist())
            gy[b, co, q[0], q[1], q[2]] = 1.0
            gx = conv3d_t2_region_dgrad(gy, w, size, crop)
            for ii, tt in reach:
                assert torch.equal(gx[b, :, ii[0], ii[1], ii[2]], w[:, co, tt[0], tt[1], tt[2]]), (k, ii)
            assert int(torch.count_nonzero(gx)) == len(reach) * cin, k
            del gx
            gx = None
            x[b, ci, i[0], i[1], i[2]] = 0.0
            gy[b, co, q[0], q[1], q[2]] = 0.0
        assert plan.tile(B - 1, last_i) == plan.tiles - 1 and q == last_o
    finally:
        del x, gy, gx
        torch.cuda.empty_cache()


# ---- routing ----
def _live_t2_geometry(n):
    """(M, full, pad, crop) of deconv_3_0 / deconv_2_0 at the live geometry of a volume of extent n."""
    from mvs_amd import regions
    from mvs_amd.config import pad_outpad
    pad, _ = pad_outpad(*n)
    full, M = regions.live_regions(n, pad)[:2]
    crop = tuple(lo - (2 * xlo - p) for (xlo, _), (lo, _), p in zip(M, full, pad))
    return M, full, pad, crop


def _count_calls(monkeypatch):
    from mvs_amd import ops
    calls = []
    for name in ("conv3d_t2_region_wgrad", "conv3d_t2_region_dgrad"):
        fn = getattr(ops, name)

        def counted(*a, _fn=fn, _name=name, **k):
            calls.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, counted)
    return calls


ROUTE_N = (24, 20, 26)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_t2_box_autograd_with_hip_backward(monkeypatch, pair):
    """regions._tconv_region -> region_train.t2_box at the live geometry of a (24, 20, 26) volume, B = 2, with
    MVS_TRAIN_T2_BWD=hip: y, gx and gw within the float64 criterion, each new op called once, the tap-GEMM backward
    never (it raises here)."""
    from mvs_amd import region_train, regions, tap_gemm
    monkeypatch.setenv("MVS_TRAIN_T2_BWD", "hip")
    monkeypatch.delenv("MVS_TRAIN_REGION_FWD", raising=False)
    monkeypatch.delenv("MVS_TRAIN_REGION_BWD", raising=False)
    M, full, pad, crop = _live_t2_geometry(ROUTE_N)
    size = tuple(regions.extent(M))
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _reference(pair, (2, size, crop, ROUTE_N), 5)
    plan = _Plan(pair, 2, size, ROUTE_N)
    print("tiles", plan.tiles)

    def refuse(*a, **k):
        raise AssertionError("the tap-GEMM backward was called")
    monkeypatch.setattr(tap_gemm, "conv_transpose3d_backward", refuse)
    calls = _count_calls(monkeypatch)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    assert region_train.t2_bwd_enabled(xg) and region_train.enabled(xg, "t2")
    y = regions._tconv_region(xg, M, wg, full, pad, ROUTE_N)
    (y * gy.to(DEV)).sum().backward()
    assert sorted(calls) == ["conv3d_t2_region_dgrad", "conv3d_t2_region_wgrad"], calls
    _check("y", y.detach(), y64, ya)
    _check("gx", xg.grad, gx64, gxa)
    _check("gw", wg.grad, gw64, gwa)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_default_t2_path_is_the_tap_gemms(monkeypatch, pair):
    """The switch unset: _tconv_region under autograd calls neither new op and its gx and gw are bit-equal to
    tap_gemm.conv_transpose3d_backward's."""
    from mvs_amd import regions, tap_gemm
    for name in ("MVS_TRAIN_T2_BWD", "MVS_TRAIN_REGION_FWD", "MVS_TRAIN_REGION_BWD", "MVS_TRAIN_S2_BWD"):
        monkeypatch.delenv(name, raising=False)
    M, full, pad, crop = _live_t2_geometry(ROUTE_N)
    size = tuple(regions.extent(M))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, pair[0], *size, generator=g).to(DEV)
    w = (torch.randn(pair[0], pair[1], 3, 3, 3, generator=g) * 0.05).to(DEV)
    gy = torch.randn(2, pair[1], *ROUTE_N, generator=g).to(DEV)
    calls = _count_calls(monkeypatch)
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = regions._tconv_region(xg, M, wg, full, pad, ROUTE_N)
    y.backward(gy)
    assert calls == []
    gx, gw = tap_gemm.conv_transpose3d_backward(x, w, 2, crop, ROUTE_N, gy)
    assert torch.equal(xg.grad, gx) and torch.equal(wg.grad, gw)


# ---- the regulariser's chain ----
def _rel(a, ref):
    ref = ref.double()
    return (a.double() - ref).norm().item() / max(ref.norm().item(), 1e-30)


CHAIN_B, CHAIN_N = 2, (16, 20, 24)   # test_regulariser_chain_with_hip_s2_backward's geometry


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
@pytest.mark.parametrize("switches", [("MVS_TRAIN_T2_BWD",),
                                      ("MVS_TRAIN_T2_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_REGION_BWD")])
def test_regulariser_chain_with_hip_t2_backward(monkeypatch, switches):
    """CostVolumeReg in train mode under autograd with the transposed layers' HIP backward -- alone, then with the
    stride-2 and stride-1 HIP backwards as well -- loss sum(P * Wr) on a random cost volume (B = 2, (16, 20, 24)):
    every parameter's gradient and the cost volume's, relative L2 to float64 forward_full <= 2 x the CPU fp32
    forward_full gradient's + 1e-5 (test_regulariser_chain_with_hip_s2_backward's bound)."""
    from conftest import record_parity
    for name in ("MVS_TRAIN_T2_BWD", "MVS_TRAIN_S2_BWD", "MVS_TRAIN_REGION_BWD", "MVS_TRAIN_REGION_FWD"):
        monkeypatch.delenv(name, raising=False)
    for name in switches:
        monkeypatch.setenv(name, "s1" if name == "MVS_TRAIN_REGION_BWD" else "hip")
    reg, cv, wr, pc, pd, cvg_c, cvg_d = _chain_reference()
    reg_g = copy.deepcopy(reg).to(DEV)
    calls = _count_calls(monkeypatch)
    cv_g = cv.to(DEV).requires_grad_(True)
    assert reg_g.live_autograd_ok(cv_g)
    (reg_g(cv_g) * wr.to(DEV)).sum().backward()
    assert sorted(calls) == ["conv3d_t2_region_dgrad"] * 2 + ["conv3d_t2_region_wgrad"] * 2, calls   # deconv_3_0, _2_0
    pg = dict(reg_g.named_parameters())
    assert all((pg[k].grad is None) == (pd[k] is None) for k in pd)
    errs = {k: (_rel(pg[k].grad.cpu(), pd[k]), _rel(pc[k], pd[k])) for k in sorted(pd) if pd[k] is not None}
    assert {"deconv_3_0.weight", "deconv_2_0.weight", "deconv_1_0.weight"} <= set(errs)
    errs["cost_volume"] = (_rel(cv_g.grad.cpu(), cvg_d), _rel(cvg_c, cvg_d))
    record_parity("region_t2_hip_backward_chain_grads_%d" % len(switches),
                  grad_rel_l2_gpu_vs_f64_max=max(v[0] for v in errs.values()),
                  grad_rel_l2_cpu_vs_f64_max=max(v[1] for v in errs.values()),
                  per_parameter={k: [float(a), float(b)] for k, (a, b) in errs.items()})
    worst = max(errs, key=lambda k: errs[k][0] / (2.0 * errs[k][1] + 1e-5))
    print("worst parameter %s: GPU %.3g, CPU fp32 %.3g, bound %.3g"
          % (worst, errs[worst][0], errs[worst][1], 2.0 * errs[worst][1] + 1e-5))
    for name, (e_g, e_c) in errs.items():
        assert e_g <= 2.0 * e_c + 1e-5, "%s: GPU grad %.3g from float64, CPU fp32 %.3g" % (name, e_g, e_c)
