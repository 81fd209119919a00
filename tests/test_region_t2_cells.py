"""The transposed region convolutions' cell kernel (csrc/conv3d_region.hip, conv3d_t2_cells_kernel): one
pass per input cell c = (o + P) >> 1, all eight output parity classes fed from registers.

ops.conv3d_region(mode=CONV_T2) runs it for 32 -> 16 channels; per_lane=True keeps the parity-class
kernel (region_conv<kT2, ..., CLS>), whose per-output accumulation order the cell kernel reproduces, so
the two must agree bit for bit.  64 -> 32 runs the class kernel either way (measured faster there), and so
does a call with y_bound (the slot a maximum lands in is that kernel's); both go through the same cases,
which hold whichever kernel the dispatch picks.

1. test_cells_equal_class_kernel: torch.equal(default, per_lane=True) on output regions chosen directly:
   every parity of (o0 + P) per dim, 1 / 17-18 / 35 cells along x (one row block + 1, three row blocks with
   a ragged tail), a region below one row block, input regions that hold every cell's inputs {c - 1, c}
   or clip them on both sides of each dim; both layer shapes, one and two inputs, both layouts, BN on
   and off, batch 1 and 3, y_bound = max|y|.
2. test_cells_impulses: one-hot inputs against the convolution's definition (output 2 i - P + t gets
   w[ci][co][t]), independent of the class kernel: every tap, both x-edge cells of a row block.
3. test_cells_float64_parity: region_cases.check_fp32 against F.conv_transpose3d in float64 on the CPU on
   the regions the regulariser forms.

The store box (st0 / stn of launch_conv3d_region) is part of the kernel's addressing but no fp32 entry
point passes one for a transposed convolution, so it has no test here.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from region_cases import GEOMETRIES, Regions, bound_of, cf, check_fp32, cl, org, size, sl, tconv_w27, zero_ext
from test_gpu_parity import _bn_params, _bn_relu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(64, 32), (32, 16)]
DIMS = [96, 96, 256]
PAD = [5, 4, 7]


def _cells(o0, on, p):
    """First cell and cell count of the outputs [o0, o0 + on) along one dim."""
    first = (o0 + p) >> 1
    return first, ((o0 + on - 1 + p) >> 1) - first + 1


def _region(par, out_size, clip):
    """(out_origin, in_origin, in_size): (out_origin + PAD) has parity `par` per dim; the input region holds
    inputs c - 1 .. c of every cell, or (clip) loses the first cell's c - 1 and the last cell's c."""
    o0, i0, isz = [], [], []
    for d in range(3):
        o = 8 + ((8 + PAD[d] + par[d]) & 1)
        first, cnt = _cells(o, out_size[d], PAD[d])
        o0.append(o)
        if clip:
            i0.append(first)
            isz.append(max(1, cnt - 1))
        else:
            i0.append(first - 1)
            isz.append(cnt + 1)
    return o0, i0, isz


SIZES = [(1, 1, 1), (2, 3, 35), (3, 2, 70), (2, 2, 5)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("two", [False, True], ids=["one_input", "two_inputs"])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_cells_equal_class_kernel(cin, cout, two, batch):
    from mvs_amd import ops
    g = torch.Generator().manual_seed(17 * cin + 3 * batch + int(two))
    w27 = tconv_w27(torch.randn(cin, cout, 3, 3, 3, generator=g) * 0.1).to(DEV)
    bn = tuple(t.to(DEV) for t in _bn_params(cout, g))
    bw = ops.bound_words(2, DEV)
    seen = set()
    for par, out_size, clip, bn_on in itertools.product(itertools.product((0, 1), repeat=3), SIZES, (False, True),
                                                        (False, True)):
        o0, i0, isz = _region(par, out_size, clip)
        assert all(((o0[d] + PAD[d]) & 1) == par[d] for d in range(3))
        seen.add((_cells(o0[2], out_size[2], PAD[2])[1], clip))
        x = torch.randn(batch, *isz, cin, generator=g).to(DEV)
        x2 = torch.randn(batch, *isz, cin, generator=g).to(DEV) if two else None
        geo = (ops.CONV_T2, DIMS, o0, list(out_size), i0, isz, PAD)
        bnd = bn if bn_on else ()
        bw.zero_()
        with torch.no_grad():
            y = ops.conv3d_region(x, x2, w27, *geo, *bnd)
            yb = ops.conv3d_region(x, x2, w27, *geo, *bnd, y_bound=bw[0])
            yp = ops.conv3d_region(x, x2, w27, *geo, *bnd, y_bound=bw[1], per_lane=True)
            yn = ops.conv3d_region(x, x2, w27, *geo, *bnd, out_ncdhw=True)
            ynp = ops.conv3d_region(x, x2, w27, *geo, *bnd, out_ncdhw=True, per_lane=True)
            torch.cuda.synchronize()
        what = (par, out_size, clip, bn_on)
        assert torch.isfinite(y).all() and (out_size == (1, 1, 1) or y.abs().max().item() > 0.0), what
        assert torch.equal(y, yp) and torch.equal(yb, yp), what
        assert torch.equal(yn, ynp), what
        assert torch.equal(yn, y.permute(0, 4, 1, 2, 3)), what
        assert bound_of(bw[0]) == bound_of(bw[1]) == y.abs().max().item(), what
    # along x: 1 cell, below one row block, one row block + 1 (17 or 18), three row blocks with a ragged tail
    counts = {c for c, _ in seen}
    assert 1 in counts and counts & {17, 18} and 35 in counts and any(1 < c < 16 for c in counts), counts


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_cells_impulses(cin, cout):
    """x[b] is one at a single (voxel, channel); w[ci][co][t] = 1 + t + 27 co (exact in fp32).  Output
    2 i - P + t of channel co must hold w[.][co][t], every other output 0."""
    from mvs_amd import ops
    out_size = (6, 6, 70)
    o0, i0, isz = _region((0, 1, 1), out_size, False)
    fx, nx = _cells(o0[2], out_size[2], PAD[2])
    assert nx > 32
    # input x positions: the first cell's c - 1 and c, cells 14 / 15 / 16 / 17 (both edges of row blocks 0 and 1:
    # input c feeds cells c and c + 1), the last cell's c; z / y interior; channels over every kq, s and block
    xs = [fx - 1, fx, fx + 14, fx + 15, fx + 16, fx + 17, fx + nx - 1]
    chans = [0, 5, 10, 15, cin - 13, cin - 1]
    pos = [(i0[0] + 2, i0[1] + 2, ix, chans[k % len(chans)]) for k, ix in enumerate(xs)]
    pos += [(i0[0] + 1 + k % 2, i0[1] + 1 + k // 2 % 2, fx + 15 + k % 3, c) for k, c in enumerate(chans)]
    batch = len(pos)
    t = torch.arange(27, dtype=torch.float32).reshape(1, 1, 3, 3, 3)
    wt = (1 + t + 27 * torch.arange(cout, dtype=torch.float32).reshape(1, cout, 1, 1, 1)).expand(cin, cout, 3, 3, 3)
    x = torch.zeros(batch, *isz, cin)
    want = torch.zeros(batch, cout, *out_size)
    taps = set()
    for b, (iz, iy, ix, c) in enumerate(pos):
        x[b, iz - i0[0], iy - i0[1], ix - i0[2], c] = 1.0
        for tz, ty, tx in itertools.product(range(3), repeat=3):
            o = [2 * i - p + tt - oo for i, p, tt, oo in zip((iz, iy, ix), PAD, (tz, ty, tx), o0)]
            if all(0 <= o[d] < out_size[d] for d in range(3)):
                want[b, :, o[0], o[1], o[2]] = wt[c, :, tz, ty, tx]
                taps.add((tz, ty, tx))
    assert len(taps) == 27
    geo = (ops.CONV_T2, DIMS, o0, list(out_size), i0, isz, PAD)
    w27 = tconv_w27(wt.contiguous()).to(DEV)
    with torch.no_grad():
        y = ops.conv3d_region(x.to(DEV), None, w27, *geo)
        yn = ops.conv3d_region(x.to(DEV), None, w27, *geo, out_ncdhw=True)
        y2 = ops.conv3d_region(torch.zeros_like(x).to(DEV), x.to(DEV), w27, *geo, out_ncdhw=True)
        torch.cuda.synchronize()
    assert torch.equal(cf(y, False), want)
    assert torch.equal(cf(yn, True), want)
    assert torch.equal(cf(y2, True), want)


@pytest.mark.parametrize("n", [(1, 2, 3), (2, 3, 4), (7, 9, 11), (6, 18, 35), (16, 5, 66)],
                         ids=lambda n: "x".join(map(str, n)))
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_cells_float64_parity(cin, cout, n):
    """deconv_3_0's (C3 -> C2) and deconv_2_0's (C2 -> B) regions of the volume n, both layer shapes on both,
    one and two inputs, both layouts, BN + ReLU."""
    from mvs_amd import ops
    assert n in GEOMETRIES
    r = Regions(n)
    batch = 1 + 2 * (GEOMETRIES.index(n) % 2)
    g = torch.Generator().manual_seed(1000 * cin + 7 * n[0] + 3 * n[1] + n[2])
    for in_reg, out_reg in ((r.C3, r.C2), (r.C2, r.B)):
        x = zero_ext(g, batch, cin, n, in_reg)
        x2 = zero_ext(g, batch, cin, n, in_reg)
        wt = torch.randn(cin, cout, 3, 3, 3, generator=g) * 0.1
        bn = _bn_params(cout, g)
        f = lambda xx, ww: _bn_relu(F.conv_transpose3d(xx, ww, stride=2, padding=r.pad, output_padding=r.outpad),
                                    *(t.to(xx.dtype) for t in bn))[sl(out_reg)]
        w27, bnd = tconv_w27(wt).to(DEV), tuple(t.to(DEV) for t in bn)
        xr, x2r = cl(x[sl(in_reg)]).to(DEV), cl(x2[sl(in_reg)]).to(DEV)
        geo = (ops.CONV_T2, list(n), org(out_reg), size(out_reg), org(in_reg), size(in_reg), list(r.pad))
        with torch.no_grad():
            y1 = ops.conv3d_region(xr, None, w27, *geo, *bnd)
            y1n = ops.conv3d_region(xr, None, w27, *geo, *bnd, out_ncdhw=True)
            y2 = ops.conv3d_region(xr, x2r, w27, *geo, *bnd)
            y2n = ops.conv3d_region(xr, x2r, w27, *geo, *bnd, out_ncdhw=True)
            torch.cuda.synchronize()
        check_fp32(cf(y1, False), f(x.double(), wt.double()), f(x, wt), "one input cl")
        check_fp32(cf(y1n, True), f(x.double(), wt.double()), f(x, wt), "one input ncdhw")
        xin = x + x2
        check_fp32(cf(y2, False), f(xin.double(), wt.double()), f(xin, wt), "two inputs cl")
        check_fp32(cf(y2n, True), f(xin.double(), wt.double()), f(xin, wt), "two inputs ncdhw")
