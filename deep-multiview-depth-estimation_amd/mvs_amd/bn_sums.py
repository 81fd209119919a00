"""Train-mode BatchNorm from sums (CostVolumeReg.forward_live_train): batch statistics from per-channel
sums over the live regions plus the closed-form contribution of the structurally constant rest."""
import torch


class _SumsFn(torch.autograd.Function):
    """(sum y, sum y^2) per channel in float64, with the backward as ONE fp32 pass
    g1 + 2 y g2 (autograd of the plain expression broadcasts the float64 gradients over the volume:
    float64 temporaries of twice its size, cfg 2 8 ms per 32-channel pass)."""

    @staticmethod
    def forward(ctx, y, cdim):
        red = [d for d in range(y.dim()) if d != cdim]
        ctx.save_for_backward(y)
        ctx.cdim = cdim
        return y.sum(red, dtype=torch.float64), (y * y).sum(red, dtype=torch.float64)

    @staticmethod
    def backward(ctx, g1, g2):
        (y,) = ctx.saved_tensors
        shape = [1] * y.dim()
        shape[ctx.cdim] = -1
        c = y.shape[ctx.cdim]
        g1 = (torch.zeros(c, dtype=y.dtype, device=y.device) if g1 is None else g1.to(y.dtype)).view(shape)
        g2 = (torch.zeros(c, dtype=y.dtype, device=y.device) if g2 is None else g2.to(y.dtype)).view(shape)
        return torch.addcmul(g1, y, 2.0 * g2), None


def _sums(y, cdim=1):
    """Per-channel sum and sum of squares of y (channels on dim cdim) in float64."""
    cdim = cdim % y.dim()
    if torch.is_grad_enabled() and y.requires_grad:
        return _SumsFn.apply(y, cdim)
    red = [d for d in range(y.dim()) if d != cdim]
    return y.sum(red, dtype=torch.float64), (y * y).sum(red, dtype=torch.float64)


def _bn_train(bn, s1, s2, count):
    """Batch statistics of a train-mode BatchNorm from per-channel sums over `count` elements:
    returns (scale, shift, mean) with BN(x) = (x - mean) * scale + shift (biased variance), and
    updates bn's running statistics the way torch's batch_norm does (unbiased variance, momentum,
    num_batches_tracked)."""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    with torch.no_grad():
        bn.num_batches_tracked.add_(1)
        m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
        bn.running_mean.mul_(1.0 - m).add_(mean.to(bn.running_mean), alpha=m)
        bn.running_var.mul_(1.0 - m).add_((var * (count / max(count - 1, 1))).to(bn.running_var), alpha=m)
    scale = bn.weight / torch.sqrt(var.to(bn.weight.dtype) + bn.eps)
    return scale, bn.bias, mean.to(bn.weight.dtype)


def _apply_bn(y, scale, shift, mean):
    v = lambda t: t.view((1, -1) + (1,) * (y.dim() - 2))
    return (y - v(mean)) * v(scale) + v(shift)


def _bn_train_hip(bn, s1, s2, count, border=None):
    """_bn_train on the HIP path as ONE launch (ops.bn_train_params), returning the [3, C] parameters
    (scale, shift, mean); ``border``: None or (weight, region, n, batch, prev) -- conv_k_1's
    border-class term (_border_class_sums) with the previous BN's parameters ``prev``.  momentum=None
    (the cumulative average) takes the device-op path."""
    from .ops import bn_train_params
    if bn.momentum is None:
        if border is not None:
            weight, reg, n, bsz, prev = border
            c1, c2 = _border_class_sums(weight, _bn_constant(tuple(prev)), reg, n, bsz)
            s1, s2 = s1 + c1, s2 + c2
        return torch.stack([t.detach().float() for t in _bn_train(bn, s1, s2, count)])
    b = None
    if border is not None:
        weight, reg, n, bsz, prev = border
        b = _border_tables_u(weight, reg, n, bsz) + (prev,)
    return bn_train_params(bn, s1, s2, count, b)


def _border_tables_u(weight, reg, n, bsz):
    """(U [C_out, C_in, K], counts [K]) of _border_class_sums for the K border classes outside reg:
    U[o][i][k] = the sum of weight[o][i] over class k's in-volume taps (float64), counts = voxels of the
    class outside reg over the batch -- cached per weight state (ops.derived), so a forward only forms
    u = U a (mvs_bn_train_params)."""
    from .ops import derived

    def build(w):
        masks, cnt, inside = _border_class_tables(tuple(n), tuple(reg), w.device)
        u = torch.einsum("oiabc,xa,yb,zc->oixyz", w.detach().double(), masks[0], masks[1], masks[2])
        outer = lambda v: v[0].view(-1, 1, 1) * v[1].view(1, -1, 1) * v[2].view(1, 1, -1)
        count = bsz * (outer(cnt) - outer(inside))
        return u.reshape(u.shape[0], u.shape[1], -1).contiguous(), count.reshape(-1).contiguous()
    return derived(("border_u", tuple(reg), tuple(n), int(bsz)), (weight,), build, weight.device)


def _bn_constant(p):
    """relu(BN(0)) per channel: the value of a BN + ReLU output where its input is exactly 0."""
    scale, shift, mean = p
    return torch.relu(-mean * scale + shift)


def _border_classes(d, lo, hi):
    """One dim of size d under a 3-tap, stride-1, padding-1 conv: (taps inside the volume, voxels
    of the class, of them inside [lo, hi]) for the border / interior index classes."""
    spans = [(0, 0, (1,))] if d == 1 else (
        [(0, 0, (1, 2)), (d - 1, d - 1, (0, 1))] + ([(1, d - 2, (0, 1, 2))] if d > 2 else []))
    return [(taps, b - a + 1, max(0, min(b, hi) - max(a, lo) + 1)) for a, b, taps in spans]


_CLASS_TABLES = {}


def _border_class_tables(n, reg, device):
    """Per dim: (tap masks [classes, 3], class voxel counts, of them inside reg) as float64 device
    tensors, cached per (volume, region, device): formed once instead of by host-to-device copies in
    every train-mode forward (pageable copies stall the host's run-ahead)."""
    key = (n, reg, str(device))
    hit = _CLASS_TABLES.get(key)
    if hit is None:
        masks, cnt, inside = [], [], []
        for d, (lo, hi) in zip(n, reg):
            classes = _border_classes(d, lo, hi)
            masks.append(torch.tensor([[1.0 if k in taps else 0.0 for k in range(3)] for taps, _, _ in classes],
                                      dtype=torch.float64, device=device))
            cnt.append(torch.tensor([c for _, c, _ in classes], dtype=torch.float64, device=device))
            inside.append(torch.tensor([i for _, _, i in classes], dtype=torch.float64, device=device))
        if len(_CLASS_TABLES) > 64:
            _CLASS_TABLES.clear()
        hit = _CLASS_TABLES[key] = (masks, cnt, inside)
    return hit


def _border_class_sums(weight, a, reg, n, bsz):
    """Sums (value, value^2) per output channel of conv3d(field, weight, padding 1) over the
    voxels OUTSIDE reg, where the input field is the per-channel constant a everywhere the
    window of such a voxel reaches (in-volume taps only).  The output there depends only on the
    voxel's border class: sum_ci a[ci] * sum_(in-volume taps) weight[co, ci, tap].  All classes
    at once (a few device ops, no per-class launches)."""
    w = weight.double()
    masks, cnt, inside = _border_class_tables(tuple(n), tuple(reg), w.device)
    # the constant field's response summed over each class's in-volume taps
    wa = torch.einsum("oiabc,i->oabc", w, a.double())    # the field's response per tap
    u = torch.einsum("oabc,zc->oabz", wa, masks[2])
    u = torch.einsum("oabz,yb->oayz", u, masks[1])
    u = torch.einsum("oayz,xa->oxyz", u, masks[0])
    outer = lambda v: v[0].view(-1, 1, 1) * v[1].view(1, -1, 1) * v[2].view(1, 1, -1)
    count = bsz * (outer(cnt) - outer(inside))            # voxels of each class outside reg
    return (u * count).sum((1, 2, 3)), (u * u * count).sum((1, 2, 3))
