"""Shared pieces of tests/test_region_geometry.py: the volume shapes, their live regions, the
zero-extended float64 references and the acceptance checks the project applies to the region kernels
(test_gpu_parity.py::test_region_conv_matches_torch, test_region_split.py::test_region_split_conv_matches_torch)."""
import numpy as np
import torch

from mvs_amd.config import pad_outpad
from mvs_amd.regions import _grow, extent, live_regions, origin

# (D, h, w): what each one hits is listed in test_region_geometry's docstring
GEOMETRIES = [(1, 2, 3), (3, 1, 5), (2, 3, 4), (5, 6, 6), (7, 9, 11), (13, 10, 17), (9, 4, 33), (16, 5, 66),
              (6, 18, 35), (20, 32, 40)]


def gid(n):
    return "x".join(str(v) for v in n)


def batch_of(n, k=0):
    """1 or 3, alternating over the geometries (and, with k, over the layers of one geometry): both
    batch sizes reach every kernel across the sweep."""
    return 1 if (GEOMETRIES.index(tuple(n)) + k) % 2 == 0 else 3


class Regions:
    """The regions CostVolumeReg._forward_live_hip and _forward_live_train_hip form for the volume n."""

    def __init__(self, n):
        self.n = tuple(n)
        self.pad, self.outpad = pad_outpad(*n)
        self.full, self.B, self.C2, self.C3 = live_regions(self.n, self.pad)
        self.hB, self.hC2, self.hC3 = (_grow(r, self.n, 1) for r in (self.B, self.C2, self.C3))
        self.M = self.B
        self.R1, self.R2 = _grow(self.M, self.n, 1), _grow(self.M, self.n, 2)


org, size = origin, extent


def sl(reg):
    return (slice(None), slice(None)) + tuple(slice(lo, hi + 1) for lo, hi in reg)


def cl(t):
    """[B, C, d, h, w] -> channels-last [B, d, h, w, C], contiguous."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def cf(y, ncdhw):
    """A kernel's region output as a CPU [B, C, d, h, w] tensor."""
    return (y if ncdhw else y.permute(0, 4, 1, 2, 3)).cpu()


def zero_ext(g, batch, c, n, reg, relu=True):
    """Values on reg, zeros on the rest of the volume n: what a region tensor stands for."""
    t = torch.zeros(batch, c, *n)
    v = torch.randn(batch, c, *extent(reg), generator=g)
    t[sl(reg)] = torch.relu(v) if relu else v
    return t


def conv_w27(wt):
    """nn.Conv3d weight [co, ci, 3, 3, 3] -> ops.region_weight's [27, co, ci]."""
    return wt.permute(2, 3, 4, 0, 1).reshape(27, wt.shape[0], wt.shape[1]).contiguous()


def tconv_w27(wt):
    """nn.ConvTranspose3d weight [ci, co, 3, 3, 3] -> [27, co, ci]."""
    return wt.permute(2, 3, 4, 1, 0).reshape(27, wt.shape[1], wt.shape[0]).contiguous()


def volume_bound_words(x):
    """int32[8] bound words of a synthetic cost volume (every |x| <= bound^2): test_split_conv._bound_words."""
    b = np.float32(np.sqrt(float(x.abs().max())) * (1 + 1e-6))
    words = torch.zeros(8, dtype=torch.int32)
    words[3] = int(np.frombuffer(b.tobytes(), dtype=np.int32)[0])
    return words


def split_volume(c4, words):
    """The split cost volume (csrc/split.h) of the fp32 channel-quad volume c4 on the host, element by
    element what test_split_cost_volume_is_the_split_of_the_fp32_volume pins: hi = fp16(v 2^e),
    lo = fp16(v 2^e - hi), stored as 4 hi then 4 lo halves per quad (int32 [B, C/4, D, h, w, 4])."""
    from mvs_amd.ops import split_exponent
    e = split_exponent(words)
    v = torch.ldexp(c4.double(), torch.tensor(float(e), dtype=torch.float64))
    hi = v.float().half()
    lo = (v - hi.double()).float().half()
    return torch.stack((hi, lo), -2).contiguous().view(torch.int32).reshape(c4.shape)


def unsplit_ncdhw(sp, words):
    """The values a split volume holds, as [B, C, D, h, w] fp32 (exact: hi + lo has at most 22 bits)."""
    from mvs_amd.ops import unsplit_cost_volume
    q = unsplit_cost_volume(sp, words)
    return q.permute(0, 1, 5, 2, 3, 4).reshape((q.shape[0], 4 * q.shape[1]) + tuple(q.shape[2:5])).contiguous()


def set_bound(row, t):
    """Bound words of a region tensor: max|t| in one slot of the zeroed row."""
    row.zero_()
    row[0] = t.abs().max().float().view(torch.int32)
    return row


def bound_of(words):
    return float(words.cpu().numpy().view(np.float32).max())


def errs(y, ref64):
    assert y.shape == ref64.shape, (tuple(y.shape), tuple(ref64.shape))
    assert torch.isfinite(y).all()
    scale = ref64.abs().max().item()
    assert scale > 0.0, "the reference is identically zero: nothing compared"
    return (y.double() - ref64).abs().max().item(), scale


def check_fp32(y, ref64, reft, what=""):
    """An fp32-MFMA / fp32 kernel: max error <= 1e-5 of the scale and <= 4x the fp32 torch (CPU)
    evaluation's own error against the same float64 reference + 1e-6 of the scale."""
    err, scale = errs(y, ref64)
    err_t = (reft.double() - ref64).abs().max().item()
    print("%s fp32: err %.3g torch-fp32 %.3g scale %.3g" % (what, err, err_t, scale))
    assert err <= 1e-5 * scale, (what, err, scale)
    assert err <= 4 * err_t + 1e-6 * scale, (what, err, err_t, scale)
    return err


def check_split(y, ref64, err32, what=""):
    """A split-fp16 kernel: max error <= 1e-5 of the scale and <= 2x the fp32 HIP kernel's on the same
    inputs + 1e-6 of the scale."""
    err, scale = errs(y, ref64)
    print("%s split: err %.3g fp32-kernel %.3g scale %.3g" % (what, err, err32, scale))
    assert err <= 1e-5 * scale, (what, err, scale)
    assert err <= 2 * err32 + 1e-6 * scale, (what, err, err32, scale)
    return err


def check_sums(s1, s2, y_own, ref64, what=""):
    """A kernel's float64 batch sums (per channel, over the whole output region):
      * against the float64 sums of the kernel's own un-boxed fp32 output y_own [B, C, ...], with
        test_region_split_sums_and_store_box's tolerance (rtol 1e-12, atol 1e-9: the same fp32 values
        added in float64, in another order);
      * against the float64 sums of the float64 reference.  The two differ by the outputs' own error,
        which check_fp32 / check_split bound by 1e-5 of the scale per element, so
        |s1 - ref1| <= N 1e-5 scale and |s2 - ref2| <= N 2.1e-5 scale^2 over the N summed elements."""
    dims = (0, 2, 3, 4)
    o1, o2 = y_own.double().sum(dims), (y_own.double() ** 2).sum(dims)
    torch.testing.assert_close(s1.cpu(), o1, rtol=1e-12, atol=1e-9, msg=lambda m: what + " s1 " + m)
    torch.testing.assert_close(s2.cpu(), o2, rtol=1e-12, atol=1e-9, msg=lambda m: what + " s2 " + m)
    scale = ref64.abs().max().item()
    count = ref64.numel() // ref64.shape[1]
    r1, r2 = ref64.sum(dims), (ref64 ** 2).sum(dims)
    assert (s1.cpu() - r1).abs().max().item() <= count * 1e-5 * scale, what
    assert (s2.cpu() - r2).abs().max().item() <= count * 2.1e-5 * scale * scale, what
