"""Live-region helpers (CostVolumeReg.forward_live).  A region is a tuple of inclusive (lo, hi) index
ranges over (D, H, W); a region tensor holds the volume's values on it.  Also the region convolutions
through PyTorch's (or, under autograd on a HIP device, tap_gemm's / region_train's) layers."""
import torch
import torch.nn.functional as F


def origin(reg):
    """The region's first index per dim, as the list the C ABI takes."""
    return [lo for lo, _ in reg]


def extent(reg):
    """The region's size per dim, as the list the C ABI takes."""
    return [hi - lo + 1 for lo, hi in reg]


def live_regions(n, pad):
    """(full, B, C2, C3): the whole volume of extent n and the regions of it that deconv_1_0,
    deconv_2_0 and deconv_3_0 read (each the transposed conv's input region of the one before)."""
    full = tuple((0, d - 1) for d in n)
    B = _tconv_input_region(full, n, pad)
    C2 = _tconv_input_region(B, n, pad)
    C3 = _tconv_input_region(C2, n, pad)
    return full, B, C2, C3


def _grow(reg, n, k):
    return tuple((max(lo - k, 0), min(hi + k, d - 1)) for (lo, hi), d in zip(reg, n))


def _tconv_input_region(out_reg, n, pad):
    """Inputs of a stride-2, kernel-3, padding-P transposed conv that reach outputs out_reg:
    input i lands on outputs 2i - P + t, t = 0..2."""
    return tuple((max(-((-(lo + p - 2)) // 2), 0), min((hi + p) // 2, d - 1))
                 for (lo, hi), d, p in zip(out_reg, n, pad))


def _crop_cf(x, x_reg, want):
    """The box `want` (inside x_reg) of a channels-first region tensor x [B, C, d, h, w], contiguous."""
    sl = [slice(lo - xlo, hi - xlo + 1) for (xlo, _), (lo, hi) in zip(x_reg, want)]
    return x[:, :, sl[0], sl[1], sl[2]].contiguous()


def _crop_cl(x, x_reg, want):
    """The box `want` (inside x_reg) of a channels-last region tensor x [B, d, h, w, C], contiguous."""
    sl = [slice(lo - xlo, hi - xlo + 1) for (xlo, _), (lo, hi) in zip(x_reg, want)]
    return x[:, sl[0], sl[1], sl[2], :].contiguous()


def _crop_pad(x, x_reg, want, n):
    """Values of the region tensor x (on x_reg) over the index box `want` (may leave the volume:
    zeros there, i.e. the conv's zero padding).  `want` inside the volume must lie in x_reg."""
    sl, pads = [], []
    for (xlo, xhi), (lo, hi), d in zip(x_reg, want, n):
        a, b = max(lo, 0), min(hi, d - 1)
        assert xlo <= a and b <= xhi, "region tensor does not cover the requested box"
        sl.append(slice(a - xlo, b - xlo + 1))
        pads.append((a - lo, hi - b))
    y = x[:, :, sl[0], sl[1], sl[2]]
    flat = [v for pr in reversed(pads) for v in pr]   # F.pad order: W, H, D
    return F.pad(y, flat) if any(flat) else y


def _taps(x):
    """The live-region helpers' convolutions go through the per-tap GEMMs (tap_gemm: MIOpen's backward
    solvers for these shapes are naive): under autograd on a HIP device in fp32."""
    return x.is_cuda and torch.is_grad_enabled() and x.dtype == torch.float32 and not torch.is_autocast_enabled()


def _region_conv3d(x, weight, stride, padding):
    if _taps(x):
        from . import tap_gemm
        return tap_gemm.conv3d(x, weight, stride, padding)
    return F.conv3d(x, weight, stride=stride, padding=padding)


def _conv_s2_region(x, weight, out_reg, pad, splits=None):
    """conv3d(x, weight, stride 2, padding pad) on the output box out_reg (x: full volume).

    Output j reads inputs 2j - P .. 2j - P + 2.  The input box of out_reg usually leaves the volume
    by different amounts on the two sides (n even); instead of materialising an asymmetrically
    padded copy, the conv runs on the in-volume crop with a symmetric padding p >= both overhangs,
    p of the left overhang's parity (so the stride-2 grid stays aligned), and the wanted outputs
    are sliced out: every kept output reads exactly its own window."""
    n = tuple(x.shape[2:])
    if _taps(x):
        # the box itself as a dense tensor: output j - lo reads inputs 2 (j - lo) - pad_lo + t of the crop
        # starting at max(2 lo - P, 0) (tap_gemm.conv3d_box)
        from . import tap_gemm
        sl, pl = [], []
        for (lo, hi), p, d in zip(out_reg, pad, n):
            a, b = 2 * lo - p, 2 * hi - p + 2
            ca, cb = max(a, 0), min(b, d - 1)
            assert ca <= cb, "output box reads no input"
            sl.append(slice(ca, cb + 1))
            pl.append(ca - a)
        whole = all(s_.start == 0 and s_.stop == d for s_, d in zip(sl, n))
        from . import region_train
        route = region_train.s2_route(x, weight, whole, splits)
        if route is not None:
            return region_train.s2_box(x, weight, out_reg, pad, tuple(pl), tuple(splits), route)
        if not whole:   # (a whole-extent slice: no copy back in the backward)
            x = x[:, :, sl[0], sl[1], sl[2]]
        return tap_gemm.conv3d_box(x, weight, 2, tuple(pl), tuple(extent(out_reg)))
    sl, pads, offs = [], [], []
    for (lo, hi), p, d in zip(out_reg, pad, n):
        a, b = 2 * lo - p, 2 * hi - p + 2
        ca, cb = max(a, 0), min(b, d - 1)
        assert ca <= cb, "output box reads no input"
        lp, rp = ca - a, b - cb
        ps = max(lp, rp)
        ps += (ps - lp) % 2
        sl.append(slice(ca, cb + 1))
        pads.append(ps)
        offs.append((ps - lp) // 2)
    y = _region_conv3d(x[:, :, sl[0], sl[1], sl[2]], weight, 2, tuple(pads))
    cnt = extent(out_reg)
    assert all(o + c <= m for o, c, m in zip(offs, cnt, y.shape[2:]))
    return y[:, :, offs[0]:offs[0] + cnt[0], offs[1]:offs[1] + cnt[1], offs[2]:offs[2] + cnt[2]]


def _conv_s1_region(x, x_reg, weight, out_reg, n):
    """conv3d(., weight, stride 1, padding 1) on out_reg, from the region tensor x on x_reg."""
    want = tuple((lo - 1, hi + 1) for lo, hi in out_reg)
    xin = _crop_pad(x, x_reg, want, n)
    from . import region_train
    route = region_train.s1_route(x, weight) if _taps(x) else None
    if route is not None:
        return region_train.s1_valid(xin, weight, route)
    return _region_conv3d(xin, weight, 1, 0)


def _tconv_region(x, x_reg, weight, out_reg, pad, dims=None):
    """conv_transpose3d(., weight, stride 2, padding pad) on out_reg, from the region tensor x on
    x_reg (which must hold every input that reaches out_reg: _tconv_input_region)."""
    if _taps(x):
        # the box as a dense tensor (tap_gemm.conv_transpose3d_box: outputs past the inputs' reach are 0)
        from . import tap_gemm
        crop = []
        for (xlo, _), (lo, hi), p in zip(x_reg, out_reg, pad):
            assert lo - (2 * xlo - p) >= 0, "transposed-conv input region starts after the output box"
            crop.append(lo - (2 * xlo - p))
        from . import region_train
        route = region_train.tconv_route(x, weight, dims is None)
        if route is not None and dims is None:
            return region_train.d1_box(x, weight, out_reg, tuple(crop))   # deconv_1_0: HIP forward and backward
        if route is not None:
            return region_train.t2_box(x, weight, x_reg, out_reg, pad, dims, tuple(crop), route)
        return tap_gemm.conv_transpose3d_box(x, weight, 2, tuple(crop), tuple(extent(out_reg)))
    y = F.conv_transpose3d(x, weight, stride=2)   # output q <-> volume index 2 * xlo + q - P
    sl, pads = [], []
    for (xlo, _), (lo, hi), p, m in zip(x_reg, out_reg, pad, y.shape[2:]):
        o0 = 2 * xlo - p
        a, b = lo - o0, hi - o0
        assert a >= 0, "transposed-conv input region starts after the output box"
        sl.append(slice(a, min(b, m - 1) + 1))
        pads.append((0, max(b - (m - 1), 0)))   # outputs past the last input's reach are 0
    y = y[:, :, sl[0], sl[1], sl[2]]
    flat = [v for pr in reversed(pads) for v in pr]
    return F.pad(y, flat) if any(flat) else y
