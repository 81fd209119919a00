"""GPU: the region convolutions' gradient kernels in the state they run in at training shapes -- several passes
of the persistent tile loop per workgroup, and element offsets past 2^31 and 2^32 bytes.

csrc/conv3d_region_wgrad.hip (stride 1, C = 16 / 32 / 64) and csrc/conv3d_s2_wgrad.hip (stacked stride 2,
32 -> 112) launch min(tiles, 168) workgroups per tap row; each walks `for (tile = chunk; tile < tiles; tile +=
chunks)` with its accumulators in registers and its LDS staging buffers reused from tile to tile.  The shapes of
test_region_train_bwd.py and test_region_train_s2_bwd.py give at most 65 and 204 tiles: the stride-1 loop never
runs a second pass there and the stride-2 loop no third.  The shapes here give every workgroup at least two
passes, most of them three or more, with a ragged last pass (tiles % 168 != 0), and the impulse tests place
their one nonzero product in a chosen pass.

The constants below MIRROR the kernels' (they are not imported: the library does not export them):
  168        kTapRowChunks (wgrad_taprow.h, the plan both kernels share), workgroups per tap row
  16         kTapRowTX, output x-voxels of a tile
  28/10/6    RwTile<C>::TR, output rows (flattened b, z, y) of a stride-1 tile for C = 16 / 32 / 64
  4/1/1      RwTile<C>::KP, partial slots per workgroup (C = 16: the four waves split the rows)
  5          kSwTR, output rows of a stride-2 tile
  tiles = ceil(Ox / 16) * ceil(B * Oz * Oy / TR)          taprow_geo
Every case first asserts, through _s1_plan / _s2_plan, that its tile count reaches the passes it is there for
and that the library's workspace size is exactly the capped one (168 slots): a change of the chunk count fails
that assertion, and no case passes while running a single pass.  (A change of TR alone moves the tile counts
asserted here against the figures in the comments: re-derive them.)

The float64 criterion is test_region_train_bwd.py's, unchanged: every element within 1e-5 x the same sum over
absolute values (+ 1e-30) of float64 F.conv3d autograd on the CPU, computed once per shape."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None

CHUNKS = 168
TILE_X = 16
S1_TR = {16: 28, 32: 10, 64: 6}
S1_KP = {16: 4, 32: 1, 64: 1}
S2_TR = 5
S2_CI, S2_CO = 32, 112


def _ints3(v):
    return (ctypes.c_int * 3)(*v)


def _cdiv(a, b):
    return -(-a // b)


class _Plan:
    """The tile walk of one launch as the kernels' *_geo functions lay it out."""

    def __init__(self, b, out, tr):
        self.out, self.tr = tuple(out), tr
        self.rows = b * out[0] * out[1]
        self.tiles_x = _cdiv(out[2], TILE_X)
        self.tiles = self.tiles_x * _cdiv(self.rows, tr)

    def tile(self, b, o):
        """Index of the tile that holds output voxel o of sample b."""
        row = (b * self.out[0] + o[0]) * self.out[1] + o[1]
        return (row // self.tr) * self.tiles_x + o[2] // TILE_X

    def pass_of(self, b, o):
        """Which iteration of its workgroup's tile loop reaches (b, o): workgroup `chunk` takes tiles chunk,
        chunk + 168, ... (all 168 workgroups exist: asserted by the plans' workspace guard)."""
        return self.tile(b, o) // CHUNKS


def _s1_plan(c, b, L, min_tiles):
    """Stride-1 plan of the padded crop L; asserts the tile count and the library's capped workspace."""
    from mvs_amd import _lib
    plan = _Plan(b, tuple(d - 2 for d in L), S1_TR[c])
    assert plan.tiles >= min_tiles and plan.tiles % CHUNKS != 0, (c, b, L, plan.tiles)
    nbytes = _lib.load().mvs_conv3d_region_wgrad_workspace_bytes(b, c, _ints3(L))
    assert nbytes == CHUNKS * S1_KP[c] * 27 * c * c * 4, (nbytes, plan.tiles)
    return plan


def _s2_plan(b, dims, out, min_tiles):
    from mvs_amd import _lib
    plan = _Plan(b, out, S2_TR)
    assert plan.tiles >= min_tiles and plan.tiles % CHUNKS != 0, (b, dims, out, plan.tiles)
    nbytes = _lib.load().mvs_conv3d_s2_region_wgrad_workspace_bytes(b, _ints3(dims), _ints3(out))
    assert nbytes == CHUNKS * 27 * S2_CO * S2_CI * 4, (nbytes, plan.tiles)
    return plan


THREE_PASSES = 2 * CHUNKS + 1   # every workgroup runs two tiles, at least one a third
TWO_PASSES = CHUNKS + 1

# ---- stride 1 ----
# (C, B, padded crop L): outputs L - 2.  (20, 19, 52): 3 * 18 * 17 = 918 rows, 50 outputs along x = 4 x-tiles, the
# last one 2 voxels wide: 153 x 4 = 612 tiles (C = 64), 92 x 4 = 368 (C = 32).  (42, 42, 38): 2 * 40 * 40 = 3200
# rows = 114 tiles of 28 rows and one of 8 (the four-wave K split meets empty rows), 36 outputs = 3 x-tiles: 345.
S1_CASES = [(64, 3, (20, 19, 52)), (32, 3, (20, 19, 52)), (16, 2, (42, 42, 38))]
S1_TILES = {64: 612, 32: 368, 16: 345}
LIVE_N = (48, 32, 40)       # the volume whose live geometry gives the model's own shapes, B = 2
S1_LIVE_TILES = {32: 206, 64: 342}   # 2 * 27 * 19 = 1026 rows, 23 outputs along x = 2 x-tiles


def _live_s1_crop(n):
    """Extent of the stride-1 layers' padded crop at the live geometry of a volume of extent n: R1 + 1 a side."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    pad, _ = pad_outpad(*n)
    M = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    return tuple(hi - lo + 3 for lo, hi in _grow(M, n, 1))


def _live_s2_geometry(n):
    """(R2, pad, pad_lo, out_size) of the stacked stride-2 layer at the live geometry of a volume of extent n."""
    from mvs_amd.config import pad_outpad
    from mvs_amd.model import _grow, _tconv_input_region
    pad, _ = pad_outpad(*n)
    M = _tconv_input_region(tuple((0, d - 1) for d in n), n, pad)
    R2 = _grow(M, n, 2)
    pl = tuple(max(2 * lo - p, 0) - (2 * lo - p) for (lo, _), p in zip(R2, pad))
    return R2, pad, pl, tuple(hi - lo + 1 for lo, hi in R2)


def _autograd64(x, w, gy, conv):
    """(y, gx, gw) of conv in float64, then the same sums over absolute values."""
    res = []
    for f in (lambda t: t.double(), lambda t: t.double().abs()):
        x64, w64 = f(x).requires_grad_(True), f(w).requires_grad_(True)
        y64 = conv(x64, w64)
        (y64 * f(gy)).sum().backward()
        res.append((y64.detach(), x64.grad, w64.grad))
    return res


@functools.lru_cache(maxsize=None)
def _s1_reference(c, b, L):
    """Inputs and the float64 CPU results of the valid stride-1 convolution, computed once per shape; the tests
    read them and leave them unchanged."""
    g = torch.Generator().manual_seed(c * 100 + b + sum(L))
    x = torch.randn(b, c, *L, generator=g)
    w = torch.randn(c, c, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, c, *[d - 2 for d in L], generator=g)
    ref, bound = _autograd64(x, w, gy, F.conv3d)
    return x, w, gy, ref, bound


def _conv64(x, w, pad_lo, out):
    """F.conv3d, stride 2, of x zero-padded by pad_lo on the low side and enough on the high side: output o
    reads inputs 2 o - pad_lo + t; the first `out` outputs per dim."""
    flat = []
    for n, p, o in reversed(list(zip(x.shape[2:], pad_lo, out))):   # F.pad order: W, H, D
        flat += [p, max(2 * o + 1 - (p + n), 0)]
    y = F.conv3d(F.pad(x, flat), w, stride=2)
    return y[:, :, :out[0], :out[1], :out[2]]


@functools.lru_cache(maxsize=None)
def _s2_reference(geo, seed):
    b, dims, pad_lo, out = geo
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, S2_CI, *dims, generator=g)
    w = torch.randn(S2_CO, S2_CI, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(b, S2_CO, *out, generator=g)
    ref, bound = _autograd64(x, w, gy, lambda a, k: _conv64(a, k, pad_lo, out))
    return x, w, gy, ref, bound


def _check(name, got, ref, bound):
    """The criterion; returns max err / (sum over absolute values), to be read against 1e-5."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got.double().cpu() - ref).abs()
    ratio = (err / (bound + 1e-30)).max().item()
    print("%s: max err %.3g, max err / bound %.3g" % (name, err.max().item(), ratio))
    assert bool((err <= 1e-5 * bound + 1e-30).all()), "%s: max err %.3g, max err / bound %.3g" % (
        name, err.max().item(), ratio)
    return ratio


def _cl(t):   # NCDHW -> channels-last, contiguous
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _s1_case_name(c, b, L):
    return "c%d_b%d_%dx%dx%d" % ((c, b) + tuple(L))


def _run_s1_case(monkeypatch, c, b, L, plan):
    """Direct ops.conv3d_region_wgrad, then region_train.s1_valid with the HIP backward, against float64."""
    from conftest import record_parity
    from mvs_amd import ops, region_train
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _s1_reference(c, b, tuple(L))
    tag = _s1_case_name(c, b, L)
    gw = ops.conv3d_region_wgrad(_cl(x.to(DEV)), _cl(gy.to(DEV)))
    r_direct = _check("direct gw " + tag, gw, gw64, gwa)

    monkeypatch.setenv("MVS_TRAIN_REGION_BWD", "s1")
    assert region_train.bwd_enabled("s1", c)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    y = region_train.s1_valid(xg, wg)
    (y * gy.to(DEV)).sum().backward()
    r_y = _check("y " + tag, y.detach(), y64, ya)
    r_gx = _check("gx " + tag, xg.grad, gx64, gxa)
    r_gw = _check("gw " + tag, wg.grad, gw64, gwa)
    assert torch.equal(wg.grad, gw)   # the same kernel on the same operands
    record_parity("region_multipass_s1_" + tag, tiles=plan.tiles, passes=_cdiv(plan.tiles, CHUNKS),
                  k_voxels=b * plan.out[0] * plan.out[1] * plan.out[2], gw_direct_err_over_sum_abs=r_direct,
                  y_err_over_sum_abs=r_y, gx_err_over_sum_abs=r_gx, gw_err_over_sum_abs=r_gw, criterion=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("c,b,L", S1_CASES)
def test_s1_three_passes_match_float64(monkeypatch, c, b, L):
    """At least three passes of the stride-1 weight gradient's tile loop with a ragged last one: gw of
    ops.conv3d_region_wgrad, and y, gx, gw of region_train.s1_valid under MVS_TRAIN_REGION_BWD=s1."""
    plan = _s1_plan(c, b, L, THREE_PASSES)
    assert plan.tiles == S1_TILES[c]
    _run_s1_case(monkeypatch, c, b, L, plan)


@pytest.mark.gpu
@pytest.mark.parametrize("c", sorted(S1_LIVE_TILES))
def test_s1_live_geometry_two_passes_match_float64(monkeypatch, c):
    """The model's own stride-1 crop at the live geometry of a (48, 32, 40) volume, B = 2: (29, 21, 25), 206
    tiles for C = 32 (two passes for 38 of the 168 workgroups), 342 for C = 64 (three passes for 6)."""
    L = _live_s1_crop(LIVE_N)
    assert L == (29, 21, 25)
    plan = _s1_plan(c, 2, L, TWO_PASSES)
    assert plan.tiles == S1_LIVE_TILES[c]
    _run_s1_case(monkeypatch, c, 2, L, plan)


# ---- stride 2 ----
# (B, dims, pad_lo, out): 3 * 14 * 14 = 588 rows = 117 tiles of 5 rows and one of 3, 40 outputs along x = 2 x-tiles
# and one of 8 voxels: 118 x 3 = 354 tiles.  The leading outputs read padding along z and x (pad_lo 1) and the
# trailing outputs reach one past the volume's end in every dim.  With pad_lo[0] = 1 the tap row tz = 0 of the
# rows oz = 0 of EVERY sample is off the volume, and so is tz = 2 of the rows oz = 13.  The point of the shape:
# sample 2's rows oz = 0 (392-405, tiles 234-245) are skipped (rowx < 0: neither gy nor x staged, the LDS rows keep
# what the workgroup's previous tile left there) in the middle of the SECOND pass and its rows oz = 13 (574-587,
# tiles 342-353) in the third, next to rows the same tile does stage -- row tile 78 holds rows 390-391 (staged)
# and 392-394 (skipped).  A skipped row that were read anyway would add the previous tile's products.
S2_GEO = (3, (27, 28, 79), (1, 0, 1), (14, 14, 40))
S2_TILES = 354


def _s2_reaches_the_end(geo):
    _, dims, pad_lo, out = geo
    return all(2 * (o - 1) - p + 1 == d - 1 for d, p, o in zip(dims, pad_lo, out))


@pytest.mark.gpu
def test_s2_three_passes_match_float64():
    """Three passes of the stride-2 weight gradient's tile loop (354 tiles) against float64, and the input
    gradient on the same operands."""
    from conftest import record_parity
    from mvs_amd import ops
    b, dims, pad_lo, out = S2_GEO
    plan = _s2_plan(b, dims, out, THREE_PASSES)
    assert plan.tiles == S2_TILES
    assert _s2_reaches_the_end(S2_GEO)   # the last output's middle tap is the volume's last voxel
    x, w, gy, (_, gx64, gw64), (_, gxa, gwa) = _s2_reference(S2_GEO, 7 + sum(dims))
    gy_cl = _cl(gy.to(DEV))
    gw = ops.conv3d_s2_region_wgrad(x.to(DEV), gy_cl, pad_lo)
    gx = ops.conv3d_s2_region_dgrad(gy_cl, w.to(DEV), dims, pad_lo)
    assert gx.is_contiguous() and tuple(gx.shape) == (b, S2_CI) + dims
    r_gw = _check("gw %s" % (S2_GEO,), gw, gw64, gwa)
    r_gx = _check("gx %s" % (S2_GEO,), gx, gx64, gxa)
    record_parity("region_multipass_s2_direct_b3_27x28x79", tiles=plan.tiles, passes=_cdiv(plan.tiles, CHUNKS),
                  k_voxels=b * out[0] * out[1] * out[2], gw_err_over_sum_abs=r_gw, gx_err_over_sum_abs=r_gx,
                  criterion=1e-5)


@pytest.mark.gpu
def test_s2_box_live_geometry_three_passes_match_float64(monkeypatch):
    """region_train.s2_box at the live geometry of a (48, 32, 40) volume, B = 2, MVS_TRAIN_S2_BWD=hip (forward on
    the tap GEMMs): the output box is 29 x 21 x 25, 2 * 29 * 21 = 1218 rows x 2 x-tiles = 488 tiles; y, gx and gw
    within the float64 criterion."""
    from conftest import record_parity
    from mvs_amd import region_train
    monkeypatch.setenv("MVS_TRAIN_S2_BWD", "hip")
    monkeypatch.delenv("MVS_TRAIN_REGION_FWD", raising=False)
    R2, pad, pl, size = _live_s2_geometry(LIVE_N)
    assert size == (29, 21, 25)
    plan = _s2_plan(2, LIVE_N, size, THREE_PASSES)
    assert plan.tiles == 488
    x, w, gy, (y64, gx64, gw64), (ya, gxa, gwa) = _s2_reference((2, LIVE_N, pl, size), 5)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    assert region_train.s2_bwd_enabled(xg) and not region_train.enabled(xg, "s2")
    y = region_train.s2_box(xg, wg, R2, pad, pl, region_train.S2_SPLITS)
    (y * gy.to(DEV)).sum().backward()
    assert xg.grad.is_contiguous()
    r_y = _check("y", y.detach(), y64, ya)
    r_gx = _check("gx", xg.grad, gx64, gxa)
    r_gw = _check("gw", wg.grad, gw64, gwa)
    record_parity("region_multipass_s2_box_live_48x32x40", tiles=plan.tiles, passes=_cdiv(plan.tiles, CHUNKS),
                  k_voxels=2 * size[0] * size[1] * size[2], y_err_over_sum_abs=r_y, gx_err_over_sum_abs=r_gx,
                  gw_err_over_sum_abs=r_gw, criterion=1e-5)


# ---- exact impulses in chosen passes ----
def _taps():
    return [(t, (t // 9, (t // 3) % 3, t % 3)) for t in range(27)]


# C = 64, B = 3, L = (20, 19, 52): outputs (18, 17, 50), row = (b * 18 + z) * 17 + y, tile = (row // 6) * 4 + x // 16
#   (0, (2, 5, 17)): row 39,  tile 6 * 4 + 1 = 25          first pass
#   (0, (15, 3, 20)): row 258, tile 43 * 4 + 1 = 173        second pass (workgroup 5's second tile)
#   (2, (17, 16, 49)): row 917, tile 152 * 4 + 3 = 611      the last tile, the 2-voxel x tile, fourth pass
S1_IMPULSE = (64, 3, (20, 19, 52))
S1_IMPULSE_VOXELS = ((0, (2, 5, 17)), (0, (15, 3, 20)), (2, (17, 16, 49)))


def _assert_passes(plan, voxels):
    """first pass, second pass, third pass or later and the very last (ragged) tile"""
    passes = [plan.pass_of(b, o) for b, o in voxels]
    assert passes[0] == 0 and passes[1] == 1 and passes[2] >= 2, passes
    assert plan.tile(*voxels[2]) == plan.tiles - 1
    assert plan.out[2] % TILE_X != 0 and voxels[2][1][2] == plan.out[2] - 1   # in the partly filled x tile


@pytest.mark.gpu
def test_s1_wgrad_tap_impulses_exact_in_each_pass():
    """test_region_wgrad_tap_impulses_exact's check at the three-pass C = 64 shape, the output voxel in a tile of
    the first pass, of the second, and in the very last tile: dw[co, ci, t] exactly -3.375, every other entry
    exactly 0.  A product from a neighbouring tile's LDS record or a tile decoded to the wrong rows breaks it."""
    from mvs_amd.ops import conv3d_region_wgrad
    c, B, L = S1_IMPULSE
    plan = _s1_plan(c, B, L, THREE_PASSES)
    _assert_passes(plan, S1_IMPULSE_VOXELS)
    O = plan.out
    x = torch.zeros((B,) + L + (c,), device=DEV)
    gy = torch.zeros((B,) + O + (c,), device=DEV)
    want = torch.zeros(c, c, 3, 3, 3, device=DEV)
    for k, (b, o) in enumerate(S1_IMPULSE_VOXELS):
        for t, (tz, ty, tx) in _taps():
            co, ci = (5 * t + 3 + k) % c, (7 * t + 11 * k) % c
            gy[b, o[0], o[1], o[2], co] = 1.5
            x[b, o[0] + tz, o[1] + ty, o[2] + tx, ci] = -2.25
            want[co, ci, tz, ty, tx] = -3.375
            dw = conv3d_region_wgrad(x, gy)
            assert torch.equal(dw, want), (k, t, dw.nonzero().tolist())
            gy[b, o[0], o[1], o[2], co] = 0.0
            x[b, o[0] + tz, o[1] + ty, o[2] + tx, ci] = 0.0
            want[co, ci, tz, ty, tx] = 0.0


# S2_GEO: out (14, 14, 40), row = (b * 14 + oz) * 14 + oy, tile = (row // 5) * 3 + ox // 16
#   (0, (1, 2, 10)): row 16,  tile 3 * 3 + 0 = 9            first pass; every tap inside the volume
#   (2, (0, 5, 20)): row 397, tile 79 * 3 + 1 = 238         second pass; oz = 0: tap row tz = 0 is off the volume
#   (2, (13, 13, 39)): row 587, tile 117 * 3 + 2 = 353      the last tile (3 rows, 8 voxels), third pass; taps 2
#                                                           are past the volume's end in every dim
S2_IMPULSE_VOXELS = ((0, (1, 2, 10)), (2, (0, 5, 20)), (2, (13, 13, 39)))


def _s2_input(o, pad_lo, tap, dims):
    i = tuple(2 * oo - p + tt for oo, p, tt in zip(o, pad_lo, tap))
    return i, all(0 <= ii < d for ii, d in zip(i, dims))


@pytest.mark.gpu
def test_s2_wgrad_tap_impulses_exact_in_each_pass():
    """test_s2_wgrad_tap_impulses_exact's check at the three-pass shape, one output voxel per pass as above, co
    in each of the three splits: dw[co, ci, t] exactly -3.375 and 0 elsewhere; a tap off the volume gives all 0
    (for tz = 0 of the second voxel the whole row is one the kernel skips, between staged rows of its tile)."""
    from mvs_amd.ops import conv3d_s2_region_wgrad
    B, dims, pad_lo, out = S2_GEO
    plan = _s2_plan(B, dims, out, THREE_PASSES)
    _assert_passes(plan, S2_IMPULSE_VOXELS)
    x = torch.zeros((B, S2_CI) + dims, device=DEV)
    gy = torch.zeros((B,) + out + (S2_CO,), device=DEV)
    want = torch.zeros(S2_CO, S2_CI, 3, 3, 3, device=DEV)
    seen, off = set(), 0
    for k, (b, o) in enumerate(S2_IMPULSE_VOXELS):
        for t, tap in _taps():
            co = (3, 20, 100)[(t + k) % 3] + (t % 5)     # < 16, 16-47, >= 48
            ci = (7 * t + 11 * k) % S2_CI
            i, inside = _s2_input(o, pad_lo, tap, dims)
            gy[b, o[0], o[1], o[2], co] = 1.5
            if inside:
                x[b, ci, i[0], i[1], i[2]] = -2.25
                want[co, ci, tap[0], tap[1], tap[2]] = -3.375
                seen.add(t)
            else:
                off += 1
            dw = conv3d_s2_region_wgrad(x, gy, pad_lo)
            assert torch.equal(dw, want), (k, t, dw.nonzero().tolist())
            gy[b, o[0], o[1], o[2], co] = 0.0
            if inside:
                x[b, ci, i[0], i[1], i[2]] = 0.0
                want[co, ci, tap[0], tap[1], tap[2]] = 0.0
    assert seen == set(range(27)) and off == 9 + 19   # voxel 2: the 9 taps tz = 0; voxel 3: all but 2 x 2 x 2


@pytest.mark.gpu
def test_s2_dgrad_impulses_exact_at_the_same_voxels():
    """test_s2_dgrad_impulses_exact's check at the three-pass shape's impulse voxels: gy = 1.0 at one (b, o, co),
    gx[b, :, 2 o - pad_lo + t] bit-equal to w[co, :, t] for the taps inside the volume and exactly 0 elsewhere."""
    from mvs_amd.ops import conv3d_s2_region_dgrad
    B, dims, pad_lo, out = S2_GEO
    _assert_passes(_s2_plan(B, dims, out, THREE_PASSES), S2_IMPULSE_VOXELS)   # the weight gradient's voxels
    w = torch.randn(S2_CO, S2_CI, 3, 3, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    gy = torch.zeros((B,) + out + (S2_CO,), device=DEV)
    for k, (b, o) in enumerate(S2_IMPULSE_VOXELS):
        want = torch.zeros((B, S2_CI) + dims, device=DEV)
        for co in (5 + k, 30 + k, 111 - k):
            hit = 0
            for t, tap in _taps():
                i, inside = _s2_input(o, pad_lo, tap, dims)
                if inside:
                    want[b, :, i[0], i[1], i[2]] = w[co, :, tap[0], tap[1], tap[2]]
                    hit += 1
            assert hit == (27, 18, 8)[k]
            gy[b, o[0], o[1], o[2], co] = 1.0
            gx = conv3d_s2_region_dgrad(gy, w, dims, pad_lo)
            gy[b, o[0], o[1], o[2], co] = 0.0
            assert torch.equal(gx, want), (k, co, (gx != want).nonzero()[:4].tolist())


# ---- bit-reproducibility across passes ----
def _poison_next_workspace(nbytes):
    """The next workspace of nbytes comes out of a block that held NaNs (test_region_train_bwd.py's step)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    poison = torch.full((2 * nbytes // 4,), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del poison


@pytest.mark.gpu
@pytest.mark.parametrize("c,b,L", S1_CASES)
def test_s1_wgrad_multipass_reproducible_whatever_the_workspace_held(c, b, L):
    from mvs_amd.ops import conv3d_region_wgrad
    _s1_plan(c, b, L, THREE_PASSES)
    g = torch.Generator(device=DEV).manual_seed(c)
    x = torch.randn((b,) + L + (c,), device=DEV, generator=g)
    gy = torch.randn((b,) + tuple(d - 2 for d in L) + (c,), device=DEV, generator=g)
    a = conv3d_region_wgrad(x, gy)
    assert torch.equal(a, conv3d_region_wgrad(x, gy))
    _poison_next_workspace(CHUNKS * S1_KP[c] * 27 * c * c * 4)
    again = conv3d_region_wgrad(x, gy)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(a, again)


@pytest.mark.gpu
def test_s2_wgrad_multipass_reproducible_whatever_the_workspace_held():
    from mvs_amd.ops import conv3d_s2_region_wgrad
    B, dims, pad_lo, out = S2_GEO
    _s2_plan(B, dims, out, THREE_PASSES)
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((B, S2_CI) + dims, device=DEV, generator=g)
    gy = torch.randn((B,) + out + (S2_CO,), device=DEV, generator=g)
    a = conv3d_s2_region_wgrad(x, gy, pad_lo)
    assert torch.equal(a, conv3d_s2_region_wgrad(x, gy, pad_lo))
    _poison_next_workspace(CHUNKS * 27 * S2_CO * S2_CI * 4)
    again = conv3d_s2_region_wgrad(x, gy, pad_lo)
    assert bool(torch.isfinite(again).all())
    assert torch.equal(a, again)


# ---- element offsets past 2^31 and 2^32 bytes: exact impulses in zero tensors, no float64 reference ----
GB = 1 << 30


def _need_free(peak_bytes):
    """Skip only where the device cannot hold the test: less free memory than its stated peak + 2 GB."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < peak_bytes + 2 * GB:
        pytest.skip("%.1f GB free on the device; the test peaks at %.1f GB and wants 2 GB beside it"
                    % (free / GB, peak_bytes / GB))


def _offset_class(nbytes):
    return 0 if nbytes < (1 << 31) else (1 if nbytes < (1 << 32) else 2)


# The smallest stride-2 volume whose x passes 2^32 bytes: B * 32 * D H W * 4 > 2^32 means B * D H W > 2^25.  The
# output box that reaches the volume's end holds B * D H W / 8 voxels of 112 floats whatever the aspect (56 bytes
# per input voxel: 1.9 GB), so the shape is chosen for x alone, as little over 2^25 as whole rows allow: B = 2,
# (64, 512, 513): 2 * 16,809,984 = 33,619,968 voxels (2^25 + 65,536; < 2^31: ops.py and the C entry point admit
# it), x = 4,303,355,904 B = 2^32 + 8,388,608; pad_lo 0, out (32, 256, 256): output 255 along x reads inputs
# 510-512, the last; gy = 2 * 32 * 256 * 256 * 112 * 4 = 1,879,048,192 B, one sample of it 0.94 GB (< 2^32 - 64,
# the input gradient's buffer descriptor).  A channel plane is 67,239,936 B: planes 0-31 (sample 0, channels
# 0-31 = offsets up to 2,151,677,952) straddle 2^31 at plane 31, sample 1's channels 0-30 lie between 2^31 and
# 2^32, and channel 31 of sample 1 (from 4,236,115,968) passes 2^32 at z = 56.02: its rows z >= 57 are above.
BIG_S2 = (2, (64, 512, 513), (0, 0, 0), (32, 256, 256))


def _s2_x_offset(dims, b, ci, i):
    return ((((b * S2_CI + ci) * dims[0] + i[0]) * dims[1] + i[1]) * dims[2] + i[2]) * 4


@pytest.mark.gpu
def test_s2_wgrad_impulses_exact_past_4gb():
    """The stride-2 weight gradient with its one nonzero x element at a byte offset below 2^31, between 2^31 and
    2^32, and above 2^32 (the last element of x), each against its gy voxel: dw exactly -3.375 at the one entry,
    0 elsewhere.  An index truncated to 32 bits reads another element (0) and loses the product.
    Peak device memory 6.3 GB: x 4.30 GB, gy 1.88 GB, the workspace 0.07 GB."""
    from mvs_amd.ops import conv3d_s2_region_wgrad
    B, dims, pad_lo, out = BIG_S2
    _need_free(int(6.3 * GB))
    plan = _s2_plan(B, dims, out, THREE_PASSES)
    assert B * S2_CI * dims[0] * dims[1] * dims[2] * 4 > 1 << 32 and B * dims[0] * dims[1] * dims[2] < 1 << 31
    last = tuple(o - 1 for o in out)
    # (b, o, tap, co, ci)
    cases = ((0, (3, 7, 20), (0, 0, 0), 9, 2),
             (1, (16, 100, 130), (2, 1, 0), 40, 5),
             (B - 1, last, (1, 1, 2), 111, S2_CI - 1))
    x = gy = None
    try:
        x = torch.zeros((B, S2_CI) + dims, device=DEV)
        gy = torch.zeros((B,) + out + (S2_CO,), device=DEV)
        want = torch.zeros(S2_CO, S2_CI, 3, 3, 3, device=DEV)
        for k, (b, o, tap, co, ci) in enumerate(cases):
            i, inside = _s2_input(o, pad_lo, tap, dims)
            assert inside and _offset_class(_s2_x_offset(dims, b, ci, i)) == k
            x[b, ci, i[0], i[1], i[2]] = -2.25
            gy[b, o[0], o[1], o[2], co] = 1.5
            want[co, ci, tap[0], tap[1], tap[2]] = -3.375
            dw = conv3d_s2_region_wgrad(x, gy, pad_lo)
            assert torch.equal(dw, want), (k, dw.nonzero().tolist())
            x[b, ci, i[0], i[1], i[2]] = 0.0
            gy[b, o[0], o[1], o[2], co] = 0.0
            want[co, ci, tap[0], tap[1], tap[2]] = 0.0
        assert _s2_x_offset(dims, B - 1, S2_CI - 1, i) == x.numel() * 4 - 4 and plan.tile(B - 1, last) == plan.tiles - 1
    finally:
        del x, gy
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_s2_dgrad_impulse_exact_past_4gb():
    """The stride-2 input gradient on the same volume, gy = 1.0 at the last output voxel of the last sample: its
    window in gx (z 62-63, y 510-511, x 510-512 of sample 1: 12 taps inside, channels 0-30 at byte offsets between
    2^31 and 2^32, channel 31 above 2^32) is bit-equal to the w rows, and gx has exactly 12 x 32 nonzeros (no
    entry of w is 0): a store whose offset wrapped modulo 2^32 lands elsewhere in gx and breaks the count.
    Peak device memory 7.3 GB: gx 4.30 GB, gy 1.88 GB, up to 1.08 GB for the count's mask."""
    from mvs_amd.ops import conv3d_s2_region_dgrad
    B, dims, pad_lo, out = BIG_S2
    _need_free(int(7.3 * GB))
    w = torch.randn(S2_CO, S2_CI, 3, 3, 3, generator=torch.Generator().manual_seed(17))
    assert bool((w != 0).all())
    w = w.to(DEV)
    b, o, co = B - 1, tuple(v - 1 for v in out), 77
    lo = tuple(2 * oo - p for oo, p in zip(o, pad_lo))
    assert lo == (62, 510, 510)
    reach = tuple(min(l + 3, d) - l for l, d in zip(lo, dims))
    assert reach == (2, 2, 3)
    assert _offset_class(_s2_x_offset(dims, b, 0, lo)) == 1 and _offset_class(_s2_x_offset(dims, b, 30, lo)) == 1
    assert _offset_class(_s2_x_offset(dims, b, S2_CI - 1, lo)) == 2
    gy = gx = None
    try:
        gy = torch.zeros((B,) + out + (S2_CO,), device=DEV)
        gy[b, o[0], o[1], o[2], co] = 1.0
        gx = conv3d_s2_region_dgrad(gy, w, dims, pad_lo)
        assert tuple(gx.shape) == (B, S2_CI) + dims and gx.is_contiguous()
        window = gx[b, :, lo[0]:lo[0] + reach[0], lo[1]:lo[1] + reach[1], lo[2]:lo[2] + reach[2]]
        assert torch.equal(window, w[co, :, :reach[0], :reach[1], :reach[2]])
        assert int(torch.count_nonzero(gx)) == reach[0] * reach[1] * reach[2] * S2_CI
    finally:
        del gy, gx
        torch.cuda.empty_cache()


# Stride 1, C = 64: x_cl [B, Lz, Ly, Lx, 64] passes 2^32 bytes when B * Lz Ly Lx > 2^24, and gy_cl is as large
# but for the halo, so the two together set the peak.  B = 2, L = (131, 258, 258), outputs (129, 256, 256):
# x_cl = 2 * 8,719,884 voxels * 256 B = 4,464,580,608 B, gy_cl = 2 * 8,454,144 * 256 = 4,328,521,728 B -- both
# over 2^32 = 4,294,967,296, so the last impulse is past 2^32 in BOTH operands (one z plane less and gy_cl ends
# exactly at 2^32).  A sample of x_cl is 2,232,290,304 B: 2^31 falls at z = 126.02 of sample 0 and 2^32 at
# z = 121.05 of sample 1.
BIG_S1 = (64, 2, (131, 258, 258))


@pytest.mark.gpu
def test_s1_wgrad_impulses_exact_past_4gb():
    """The stride-1 C = 64 weight gradient with its one nonzero x element below 2^31 bytes, between 2^31 and 2^32,
    and above 2^32 (the last element of x_cl, against the last element of gy_cl, also past 2^32): dw exactly
    -3.375 at the one entry, 0 elsewhere.
    Peak device memory 8.9 GB: x_cl 4.46 GB, gy_cl 4.33 GB, the workspace 0.07 GB."""
    from mvs_amd.ops import conv3d_region_wgrad
    c, B, L = BIG_S1
    _need_free(int(8.9 * GB))
    plan = _s1_plan(c, B, L, THREE_PASSES)
    O = plan.out
    assert B * L[0] * L[1] * L[2] * c * 4 > 1 << 32 and B * L[0] * L[1] * L[2] < 1 << 31
    last = tuple(d - 1 for d in O)
    # (b, o, tap, co, ci)
    cases = ((0, (4, 9, 33), (0, 0, 0), 6, 50),
             (0, (126, 200, 77), (1, 2, 0), 35, 17),
             (B - 1, last, (2, 2, 2), c - 1, c - 1))

    def x_offset(b, o, tap, ci):
        i = tuple(a + t for a, t in zip(o, tap))
        return ((((b * L[0] + i[0]) * L[1] + i[1]) * L[2] + i[2]) * c + ci) * 4

    x = gy = None
    try:
        x = torch.zeros((B,) + L + (c,), device=DEV)
        gy = torch.zeros((B,) + O + (c,), device=DEV)
        want = torch.zeros(c, c, 3, 3, 3, device=DEV)
        for k, (b, o, (tz, ty, tx), co, ci) in enumerate(cases):
            assert _offset_class(x_offset(b, o, (tz, ty, tx), ci)) == k
            x[b, o[0] + tz, o[1] + ty, o[2] + tx, ci] = -2.25
            gy[b, o[0], o[1], o[2], co] = 1.5
            want[co, ci, tz, ty, tx] = -3.375
            dw = conv3d_region_wgrad(x, gy)
            assert torch.equal(dw, want), (k, dw.nonzero().tolist())
            x[b, o[0] + tz, o[1] + ty, o[2] + tx, ci] = 0.0
            gy[b, o[0], o[1], o[2], co] = 0.0
            want[co, ci, tz, ty, tx] = 0.0
        assert x_offset(B - 1, last, (2, 2, 2), c - 1) == x.numel() * 4 - 4 and gy.numel() * 4 > 1 << 32
        assert plan.tile(B - 1, last) == plan.tiles - 1
    finally:
        del x, gy
        torch.cuda.empty_cache()
