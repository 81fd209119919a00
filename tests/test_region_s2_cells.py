"""The stride-2 region convolution's cell kernel (csrc/conv3d_region.hip, conv3d_s2_cells_kernel): a GEMM row is
a cell of CZ x CY outputs in (z, y) at one output x, whose (2 CZ + 1) x (2 CY + 1) input rows are loaded once and
fed to every accumulator that reads them.

ops.conv3d_region(mode=CONV_S2) runs it for 32 -> 16 channels from the fp32 volume (NCDHW or channel quads);
per_lane=True keeps the per-lane kernel (region_conv<kS2>), whose per-output accumulation order the cell kernel
reproduces, so the two must agree bit for bit.  32 -> 32 and 32 -> 64 run the per-lane kernel either way and go
through the same cases, which hold whichever kernel the dispatch picks.

1. test_s2_cell_grid_matches_enumeration (CPU): the launch geometry (mvs_conv3d_s2_cells_geometry) against a
   brute-force enumeration of cells, and the (c_in, c_out) pairs it reports as dispatched.
2. test_cells_equal_per_lane_kernel: torch.equal(default, per_lane=True) on regions chosen directly: extents
   1, 2, 3, 5 along z and y (a lone cell, a full one, a clipped last one, per dim), 1, 3, 18, 35 along x (a
   partial row block, one block and a tail, blocks that straddle cell lines), origins of both parities per dim,
   odd and even volumes with pad = n // 2 + 1 (taps off every face), a cv_box smaller than the volume, both
   input layouts, BN on and off, both output layouts, batch 1 and 3.
3. test_cells_impulses: one-hot inputs against the convolution's definition, independent of the per-lane
   kernel: every one of the 27 taps at every corner output of a cell.
4. test_cells_float64_parity: against F.conv3d in float64 on the CPU with the existing stride-2 region tests'
   tolerance (1e-5 sum|x||w| |scale| + the BN epilogue's rounding).
"""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from region_cases import conv_w27
from test_gpu_parity import _bn_params, _to_c4

DEV = torch.device("cuda:0")
PAIRS = [(32, 16), (32, 32), (32, 64)]
CELL_PAIRS = {(32, 16)}   # the pairs the cell kernel is instantiated for


def _geometry(cin, cout, size):
    from mvs_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_longlong * 6)()
    st = lib.mvs_conv3d_s2_cells_geometry(cin, cout, (ctypes.c_int * 3)(*size), out)
    return st, list(out)


def test_s2_cell_grid_matches_enumeration():
    """rows, waves and workgroups of the launch against an enumeration of the cells: every output (z, y, x)
    belongs to exactly one (cell, x) row; rows fill 16-row blocks, RB blocks a wave, 4 waves a workgroup, the
    workgroup count rounded up to the 8 XCDs."""
    sizes = [(1, 1, 1), (2, 2, 3), (3, 5, 18), (5, 3, 35), (5, 5, 1), (7, 9, 83), (50, 34, 42), (98, 66, 83)]
    for size in sizes:
        st, (cz, cy, rb, rows, waves, blocks) = _geometry(32, 16, size)
        assert st == 1 and cz >= 1 and cy >= 1 and rb >= 1
        cells = {(z // cz, y // cy) for z in range(size[0]) for y in range(size[1])}
        seen = {}
        for z, y, x in itertools.product(*(range(s) for s in size)):
            row = ((z // cz) * ((size[1] + cy - 1) // cy) + y // cy) * size[2] + x
            seen.setdefault(row, []).append((z % cz, y % cy))
        assert rows == len(cells) * size[2] == len(seen) and max(seen) == rows - 1, size
        assert all(len(set(v)) == len(v) <= cz * cy for v in seen.values())
        want_waves = -(-rows // (16 * rb))
        assert waves == want_waves, size
        assert blocks == 8 * -(-(-(-want_waves // 4)) // 8) and blocks * 4 >= waves, size
    # the instantiated pairs are the dispatched ones; other shapes report 0 and an invalid size -1
    for pair in PAIRS + [(16, 16), (64, 32)]:
        assert _geometry(*pair, (3, 3, 3))[0] == (1 if pair in CELL_PAIRS else 0), pair
    assert _geometry(32, 16, (0, 3, 3))[0] == -1


def _case(n, o0, on):
    """pad = n // 2 + 1 per dim (config.py); the region must lie in the convolution's output range."""
    pad = [d // 2 + 1 for d in n]
    outn = [(d + 2 * p - 3) // 2 + 1 for d, p in zip(n, pad)]
    assert all(0 <= a and a + k <= m for a, k, m in zip(o0, on, outn)), (n, o0, on, outn)
    return pad


def _reach(n, pad, o0, on):
    """Per dim: does a window of the region straddle the low / the high face of the volume (taps on both sides)?"""
    return [(2 * a - p < 0 <= 2 * a - p + 2, 2 * (a + k - 1) - p <= d - 1 < 2 * (a + k - 1) - p + 2)
            for a, k, p, d in zip(o0, on, pad, n)]


# (volume, region origin, region size): every z / y extent of {1, 2, 3, 5}, every x extent of {1, 3, 18, 35}
# (35 outputs along x need a volume of 2 * 35 voxels and more), origins of both parities per dim.  With
# pad = n // 2 + 1 only the outputs (P - 2) / 2 .. (n - 1 + P) / 2 have a tap inside the volume (the middle half
# of each dim), so the regions sit at the two ends of that range, where the windows straddle the faces
REGIONS = [
    ((12, 10, 38), (3, 2, 9), (1, 2, 1)),
    ((12, 10, 38), (8, 7, 26), (2, 1, 3)),
    ((12, 10, 38), (3, 2, 10), (3, 5, 18)),
    ((12, 10, 38), (4, 3, 11), (5, 3, 18)),
    ((12, 10, 38), (5, 6, 9), (5, 2, 3)),
    ((11, 9, 37), (2, 2, 9), (5, 5, 18)),
    ((11, 9, 37), (4, 3, 10), (5, 3, 18)),
    ((11, 9, 37), (3, 2, 25), (3, 3, 3)),
    ((7, 10, 72), (1, 2, 18), (2, 5, 35)),
    ((6, 9, 71), (2, 3, 19), (3, 2, 35)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_cells_equal_per_lane_kernel(cin, cout, batch):
    from mvs_amd import ops
    g = torch.Generator().manual_seed(31 * cout + batch)
    w27 = conv_w27(torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bn = tuple(t.to(DEV) for t in _bn_params(cout, g))
    faces, extents, parities = set(), [set(), set(), set()], set()
    for (n, o0, on), boxed, bn_on in itertools.product(REGIONS, (False, True), (False, True)):
        pad = _case(n, o0, on)
        for d, (lo, hi) in enumerate(_reach(n, pad, o0, on)):
            faces |= {(d, "lo")} if lo else set()
            faces |= {(d, "hi")} if hi else set()
            extents[d].add(on[d])
        parities.add(tuple(a & 1 for a in o0))
        x = torch.randn(batch, cin, *n, generator=g)
        if boxed:   # the tensor holds a box of the volume that cuts the region's windows on every side it can
            i0 = [max(0, 2 * a - p + 1) for a, p in zip(o0, pad)]
            i1 = [min(d, max(lo + 1, 2 * (a + k - 1) - p + 2)) for a, k, p, d, lo in zip(o0, on, pad, n, i0)]
            isz = [b - a for a, b in zip(i0, i1)]
            xb = x[:, :, i0[0]:i1[0], i0[1]:i1[1], i0[2]:i1[2]].contiguous()
            box = (i0, isz)
        else:
            xb, box = x, (None, None)
        geo = (ops.CONV_S2, list(n), list(o0), list(on), *box, pad)
        bnd = bn if bn_on else ()
        xd, x4 = xb.to(DEV), _to_c4(xb.to(DEV))
        with torch.no_grad():
            y = ops.conv3d_region(xd, None, w27, *geo, *bnd)
            yp = ops.conv3d_region(xd, None, w27, *geo, *bnd, per_lane=True)
            y4 = ops.conv3d_region(x4, None, w27, *geo, *bnd, in_c4=True)
            y4p = ops.conv3d_region(x4, None, w27, *geo, *bnd, in_c4=True, per_lane=True)
            yn = ops.conv3d_region(x4, None, w27, *geo, *bnd, in_c4=True, out_ncdhw=True)
            ynp = ops.conv3d_region(x4, None, w27, *geo, *bnd, in_c4=True, out_ncdhw=True, per_lane=True)
            torch.cuda.synchronize()
        what = (n, o0, on, boxed, bn_on)
        assert y.shape == (batch, *on, cout) and torch.isfinite(y).all() and y.abs().max().item() > 0.0, what
        assert torch.equal(y, yp), what
        assert torch.equal(y4, y4p) and torch.equal(y4, y), what
        assert torch.equal(yn, ynp) and torch.equal(yn, y.permute(0, 4, 1, 2, 3)), what
    assert faces == {(d, s) for d in range(3) for s in ("lo", "hi")}, faces
    assert extents[0] >= {1, 2, 3, 5} and extents[1] >= {1, 2, 3, 5} and extents[2] >= {1, 3, 18, 35}, extents
    assert all({p[d] for p in parities} == {0, 1} for d in range(3)), parities


@pytest.mark.gpu
@pytest.mark.parametrize("c4", [True, False], ids=["quads", "ncdhw"])
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_cells_impulses(cin, cout, c4):
    """x[b] is one at a single (voxel, channel); w[co][ci][t] = 1 + t + 27 co (exact in fp32).  Output o with
    2 o - P + t = the voxel must hold w[co][.][t], every other output 0.  The voxels are the 27 inputs
    2 o - P + t of a cell-corner output o (cells of up to 4 x 4 start at multiples of 4 of the region), once per
    corner parity in (z, y), so every tap reaches an output in every position of a cell."""
    from mvs_amd import ops
    n = (16, 18, 40)
    pad = [d // 2 + 1 for d in n]
    o0, on = [2, 3, 1], [9, 9, 18]
    corners = [(o0[0] + 4 + dz, o0[1] + 4 + dy, o0[2] + 15 + dz) for dz, dy in itertools.product((0, 1), repeat=2)]
    pos = []
    for k, (corner, t) in enumerate(itertools.product(corners, itertools.product(range(3), repeat=3))):
        if k % 4 == (t[0] + t[1]) % 4 or t == (1, 1, 1):   # a quarter of each corner's taps: all 27 over the four
            pos.append(tuple(2 * o - p + tt for o, p, tt in zip(corner, pad, t)) + ((5 * k + 3) % cin,))
    batch = len(pos)
    t = torch.arange(27, dtype=torch.float32).reshape(1, 1, 3, 3, 3)
    wt = (1 + t + 27 * torch.arange(cout, dtype=torch.float32).reshape(cout, 1, 1, 1, 1)).expand(cout, cin, 3, 3, 3)
    x = torch.zeros(batch, cin, *n)
    want = torch.zeros(batch, *on, cout)
    taps, cellpos = set(), set()
    for b, (iz, iy, ix, c) in enumerate(pos):
        assert all(0 <= i < d for i, d in zip((iz, iy, ix), n))
        x[b, c, iz, iy, ix] = 1.0
        for tz, ty, tx in itertools.product(range(3), repeat=3):
            num = [i + p - tt for i, p, tt in zip((iz, iy, ix), pad, (tz, ty, tx))]
            if any(v % 2 for v in num):
                continue
            o = [v // 2 - a for v, a in zip(num, o0)]
            if all(0 <= o[d] < on[d] for d in range(3)):
                want[b, o[0], o[1], o[2], :] = wt[:, c, tz, ty, tx]
                taps.add((tz, ty, tx))
                cellpos.add((tz, ty, tx, o[0] % 2, o[1] % 2))
    assert len(taps) == 27 and len(cellpos) >= 27 * 2
    geo = (ops.CONV_S2, list(n), o0, on, None, None, pad)
    w27 = conv_w27(wt.contiguous()).to(DEV)
    xin = _to_c4(x.to(DEV)) if c4 else x.to(DEV)
    with torch.no_grad():
        y = ops.conv3d_region(xin, None, w27, *geo, in_c4=c4)
        yn = ops.conv3d_region(xin, None, w27, *geo, in_c4=c4, out_ncdhw=True)
        torch.cuda.synchronize()
    assert torch.equal(y.cpu(), want)
    assert torch.equal(yn.cpu(), want.permute(0, 4, 1, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True])
def test_cells_float64_parity(bn):
    """conv_1_0's shape (32 -> 16) on regions with odd extents and both input layouts against a float64
    convolution: |err| <= 1e-5 sum|x||w| |scale| + 1e-6 (|mu scale| + |shift|), the tolerance of
    test_gpu_parity.py's stride-2 region tests."""
    from mvs_amd import ops
    g = torch.Generator().manual_seed(77 + bn)
    for (n, o0, on), batch in zip((REGIONS[2], REGIONS[5], REGIONS[8]), (2, 1, 1)):
        pad = _case(n, o0, on)
        x = torch.randn(batch, 32, *n, generator=g)
        wt = torch.randn(16, 32, 3, 3, 3, generator=g) * 0.1
        p1 = _bn_params(16, g) if bn else None
        p1d = [t.to(DEV) for t in p1] if bn else []
        geo = (ops.CONV_S2, list(n), list(o0), list(on), None, None, pad)
        with torch.no_grad():
            y = ops.conv3d_region(x.to(DEV), None, conv_w27(wt).to(DEV), *geo, *p1d)
            y4 = ops.conv3d_region(_to_c4(x.to(DEV)), None, conv_w27(wt).to(DEV), *geo, *p1d, in_c4=True)
        sl = (slice(None),) * 2 + tuple(slice(lo, lo + k) for lo, k in zip(o0, on))
        ref = F.conv3d(x.double(), wt.double(), stride=2, padding=pad)[sl]
        aref = F.conv3d(x.double().abs(), wt.double().abs(), stride=2, padding=pad)[sl]
        bnmag = 0.0
        if bn:
            sc, sh, mu = [t.double().view(1, -1, 1, 1, 1) for t in p1]
            ref = torch.relu((ref - mu) * sc + sh)
            aref = aref * sc.abs()
            bnmag = ((mu * sc).abs() + sh.abs()).permute(0, 2, 3, 4, 1)
        ref, aref = ref.permute(0, 2, 3, 4, 1), aref.permute(0, 2, 3, 4, 1)
        tol = 1e-5 * aref + 1e-6 * bnmag + 1e-30
        for name, got in (("ncdhw", y), ("quads", y4)):
            err = (got.double().cpu() - ref).abs()
            assert bool((err <= tol).all()), "%s %s: max err %.3g" % (name, n, err.max().item())
