"""Forward + backward time of one layer family of the train step, each layer alone at the shapes of one cfg-2 step
(B = 4, the (192, 128, 160) cost volume, the live regions of regions.live_regions), with the family's training switch
at its default against its HIP value (mvs_amd/train_switches.py), the two alternated --runs times; then the peak
memory of one forward + backward for both, and the HIP kernels on their own against a bound.

  family   switch                       layers                                      bound on the kernels alone
  s1       MVS_TRAIN_REGION_BWD=s1      conv_1_1 / conv_2_1 / conv_3_1 (s1_valid)   weight gradient: share of f32 matrix peak
  s2       MVS_TRAIN_S2_BWD=hip         stacked conv_k_0, 32 -> 16 + 32 + 64        both gradients: share of f32 matrix peak
  t2       MVS_TRAIN_T2_BWD=hip         deconv_3_0, deconv_2_0 (x, gy channels-last) both gradients: share of f32 matrix peak
  deconv1  MVS_TRAIN_DECONV1=hip        deconv_1_0 (x channels-last, gy NCDHW)      x one-pass HBM time
  bn       MVS_TRAIN_BN=hip             the y0 site and deconv_3_0's output site    x five-pass HBM time
  conv2d   MVS_TRAIN_CONV2D_BWD=hip     8 encoder + 4 refinement Conv2d layers      one-pass HBM time beside each kernel

The operands are in the memory layouts they have inside the train step.  bn and conv2d call the two
implementations directly (the torch passes / tap_gemm.conv2d_hip_fwd against bn_train.bn_relu_train /
conv2d_train.conv2d_hip): what the switch chooses between.  The FLOP rates count 2 * 27 * c_in * c_out per voxel
(t2: per input voxel, taps that land outside the box included: an upper bound of a few percent).

Usage: python tools/train_layer_ab.py --family F [--reps N] [--runs N] [--batch B] [--dims D H W]
       (one JSON line per layer, the keys of the profiles/*_layers_cfg2.txt / *_sites_cfg2.txt files)"""
import argparse
import collections
import contextlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "deep-multiview-depth-estimation_amd"))
import torch  # noqa: E402
from mvs_amd import bn_train, conv2d_train, model, ops, region_train, regions, tap_gemm, train_switches  # noqa: E402
from mvs_amd.bn_sums import _apply_bn, _bn_train, _sums  # noqa: E402
from mvs_amd.config import pad_outpad  # noqa: E402

PEAK_F32_MATRIX_TF = 157.3
HBM_COPY_TBS = 6.29   # measured copy ceiling

# row: the JSON line's leading keys.  sides: ((label, switch value or None, forward + backward closure), the same for
# "hip"); with a switch value the closure runs under FAMILY.switch = value.  reset: drops the gradients.  alone: adds
# the stand-alone kernel times and the bound to the row.
Layer = collections.namedtuple("Layer", "row sides reset alone")
# peak: None, "GB" (max_memory_allocated) or "MB" (above the layer's own tensors)
Family = collections.namedtuple("Family", "switch peak layers")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ms(fn, reps):
    return round(timed(fn, reps), 4)


Geometry = collections.namedtuple("Geometry", "batch n pad full M size crop")


def geometry(a):
    """The cfg-2 live geometry: the volume extent n, the region M the transposed layers read, its extent, and their
    crop of the full box."""
    n = tuple(a.dims)
    pad, _ = pad_outpad(*n)
    full, M = regions.live_regions(n, pad)[:2]
    crop = tuple(lo - (2 * xlo - p) for (xlo, _), (lo, _), p in zip(M, full, pad))
    return Geometry(a.batch, n, pad, full, M, tuple(regions.extent(M)), crop)


def cl(shape, dev, rand=torch.randn):
    """A logical NCDHW tensor over channels-last memory."""
    return rand((shape[0],) + tuple(shape[2:]) + (shape[1],), device=dev).permute(0, 4, 1, 2, 3)


def weight(*shape, dev):
    return (torch.randn(*shape, device=dev) * 0.05).requires_grad_(True)


@contextlib.contextmanager
def switched(name, value):
    if name is None or value is None:
        yield
        return
    os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name)


def matrix_peak_share(row, flop, kernels):
    for k in kernels:
        tf = flop / (row["hip_%s_ms" % k] * 1e-3) / 1e12
        row["hip_%s_TF" % k] = round(tf, 2)
        row["hip_%s_share_of_f32_matrix_peak" % k] = round(tf / PEAK_F32_MATRIX_TF, 4)


def hbm_ms(nbytes):
    return nbytes / (HBM_COPY_TBS * 1e12) * 1e3


def _switch_sides(fwd_bwd, on):
    return (("taps", "taps", fwd_bwd), ("hip", on, fwd_bwd))


def s1_layers(g, dev, reps):
    R1 = regions._grow(g.M, g.n, 1)
    L = [e + 2 for e in regions.extent(R1)]   # the zero-padded crop _conv_s1_region hands s1_valid
    out = [d - 2 for d in L]
    for c in region_train.S1_CHANNELS:
        x = torch.randn([g.batch, c] + L, device=dev, requires_grad=True)
        w = weight(c, c, 3, 3, 3, dev=dev)
        gy = torch.randn([g.batch, c] + out, device=dev)

        def reset():
            x.grad = w.grad = None

        def fwd_bwd():
            reset()
            region_train.s1_valid(x, w).backward(gy)

        def alone(row):
            with torch.no_grad():
                x_cl = x.detach().permute(0, 2, 3, 4, 1).contiguous()
                gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
                wa = region_train._region_w_adjoint(w)
                row["forward_ms"] = ms(lambda: region_train.s1_valid(x.detach(), w.detach()), reps)
                row["hip_gw_ms"] = ms(lambda: ops.conv3d_region_wgrad(x_cl, gy_cl), reps)
                row["hip_gx_ms"] = ms(lambda: ops.conv3d_region(gy_cl, None, wa, ops.CONV_S1, L, [0, 0, 0], L, [1, 1, 1],
                                                                out, None, per_lane=True), reps)
            matrix_peak_share(row, 2.0 * 27 * c * c * row["out_voxels"], ("gw",))
        yield Layer({"layer": "conv s1 C=%d" % c, "x": list(x.shape), "out_voxels": gy.numel() // c},
                    _switch_sides(fwd_bwd, "s1"), reset, alone)


def s2_layers(g, dev, reps):
    R2 = regions._grow(g.M, g.n, 2)
    size = tuple(regions.extent(R2))
    pl = tuple(max(2 * lo - p, 0) - (2 * lo - p) for (lo, _), p in zip(R2, g.pad))
    x = torch.rand((g.batch, 32) + g.n, device=dev, requires_grad=True)
    w = weight(112, 32, 3, 3, 3, dev=dev)
    gy = torch.randn((g.batch, 112) + size, device=dev)
    layer = lambda xx, ww: regions._conv_s2_region(xx, ww, R2, g.pad, splits=region_train.S2_SPLITS)

    def reset():
        x.grad = w.grad = None

    def fwd_bwd():
        reset()
        layer(x, w).backward(gy)

    def alone(row):
        with torch.no_grad():
            gy_cl = gy.permute(0, 2, 3, 4, 1).contiguous()
            xd, wd = x.detach(), w.detach()
            row["forward_ms"] = ms(lambda: layer(xd, wd), reps)
            row["hip_gw_ms"] = ms(lambda: ops.conv3d_s2_region_wgrad(xd, gy_cl, pl), reps)
            row["hip_gx_ms"] = ms(lambda: ops.conv3d_s2_region_dgrad(gy_cl, wd, g.n, pl), reps)
        matrix_peak_share(row, 2.0 * 27 * 32 * 112 * row["out_voxels"], ("gw", "gx"))
    yield Layer({"layer": "conv s2 32 -> 16 + 32 + 64", "x": list(x.shape), "box": list(size), "pad_lo": list(pl),
                 "out_voxels": g.batch * size[0] * size[1] * size[2]}, _switch_sides(fwd_bwd, "hip"), reset, alone)


def t2_layers(g, dev, reps):
    for name, (cin, cout) in zip(("deconv_3_0", "deconv_2_0"), region_train.T2_SHAPES):
        x = cl((g.batch, cin) + g.size, dev, torch.rand).requires_grad_(True)
        w = weight(cin, cout, 3, 3, 3, dev=dev)
        gy = cl((g.batch, cout) + g.n, dev)

        def reset():
            x.grad = w.grad = None

        def fwd_bwd():
            reset()
            regions._tconv_region(x, g.M, w, g.full, g.pad, g.n).backward(gy)

        def alone(row):
            xd, wd = x.detach(), w.detach()
            # (grad mode on: _tconv_region takes the HIP region kernel only under autograd)
            row["forward_ms"] = ms(lambda: regions._tconv_region(xd, g.M, wd, g.full, g.pad, g.n), reps)
            with torch.no_grad():
                row["hip_gw_ms"] = ms(lambda: ops.conv3d_t2_region_wgrad(xd, gy, g.crop), reps)
                row["hip_gx_ms"] = ms(lambda: ops.conv3d_t2_region_dgrad(gy, wd, g.size, g.crop), reps)
            matrix_peak_share(row, 2.0 * 27 * cin * cout * row["in_voxels"], ("gw", "gx"))
        yield Layer({"layer": "%s %d -> %d" % (name, cin, cout), "x": list(x.shape), "box": list(g.n),
                     "crop": list(g.crop), "in_voxels": g.batch * g.size[0] * g.size[1] * g.size[2]},
                    _switch_sides(fwd_bwd, "hip"), reset, alone)


def deconv1_layers(g, dev, reps):
    cin, cout = region_train.D1_SHAPE
    x = cl((g.batch, cin) + g.size, dev, torch.rand).requires_grad_(True)
    w = weight(cin, cout, 3, 3, 3, dev=dev)
    gy = torch.randn((g.batch, cout) + g.n, device=dev)
    in_vox, out_vox = g.batch * g.size[0] * g.size[1] * g.size[2], g.batch * g.n[0] * g.n[1] * g.n[2]

    def reset():
        x.grad = w.grad = None

    def fwd_bwd():
        reset()
        regions._tconv_region(x, g.M, w, g.full, g.pad).backward(gy)

    def alone(row):
        xd, wd = x.detach(), w.detach()
        x_cl = xd.permute(0, 2, 3, 4, 1)
        with torch.no_grad():
            times = {"fwd": timed(lambda: ops.deconv3d_k3s2(x_cl, [0, 0, 0], wd, list(g.n), list(g.crop), None, None,
                                                            None, None, channels_last=True), reps),
                     "gw": timed(lambda: ops.deconv3d_k3s2_wgrad(xd, gy, g.crop), reps),
                     "gx": timed(lambda: ops.deconv3d_k3s2_dgrad(gy, wd, g.size, g.crop, channels_last=True), reps)}
        nbytes = 4.0 * cin * in_vox + 4.0 * cout * out_vox   # every kernel: x and y (or gy) once each
        for k in ("fwd", "gw", "gx"):
            row["hip_%s_ms" % k] = round(times[k], 4)
            row["hip_%s_MB" % k] = round(nbytes / 1e6, 1)
            row["hip_%s_one_pass_hbm_ms" % k] = round(hbm_ms(nbytes), 4)
            row["hip_%s_x_hbm_time" % k] = round(times[k] / hbm_ms(nbytes), 2)
    yield Layer({"layer": "deconv_1_0 %d -> %d" % (cin, cout), "x": list(x.shape), "box": list(g.n),
                 "crop": list(g.crop), "in_voxels": in_vox}, _switch_sides(fwd_bwd, "hip"), reset, alone)


def bn_layers(g, dev, reps):
    count = g.batch * g.n[0] * g.n[1] * g.n[2]
    for name, c, chl, box in (("y0", 8, False, None), ("deconv_3_0 output", 32, True, g.M)):
        bn = torch.nn.BatchNorm3d(c, device=dev).train()
        z = (cl((g.batch, c) + g.n, dev) if chl else torch.randn((g.batch, c) + g.n, device=dev)).requires_grad_(True)
        gy = torch.randn((g.batch, c) + tuple(regions.extent(box if box is not None else g.full)), device=dev)

        def reset():
            z.grad = bn.weight.grad = bn.bias.grad = None

        def torch_site():
            reset()
            p = _bn_train(bn, *_sums(z), count)
            y = torch.relu(_apply_bn(z if box is None else regions._crop_pad(z, g.full, box, g.n), *p))
            y.backward(gy)

        def hip_site():
            reset()
            bn_train.bn_relu_train(z, box, bn, None, count)[0].backward(gy)
        nbytes = 4.0 * z.numel()

        def alone(row):
            # five passes over z: read for the sums, read + write for the BN; backward two reads, one write of gz
            row["five_pass_hbm_ms"] = round(5.0 * hbm_ms(nbytes), 4)
            row["hip_x_five_pass_hbm_time"] = round(min(row["hip_ms"]) / row["five_pass_hbm_ms"], 2)
            row["torch_x_five_pass_hbm_time"] = round(min(row["torch_ms"]) / row["five_pass_hbm_ms"], 2)
        yield Layer({"site": name, "z": list(z.shape), "channels_last": chl, "box": None if box is None else list(box),
                     "MB": round(nbytes / 1e6, 1)}, (("torch", None, torch_site), ("hip", None, hip_site)), reset, alone)


def conv2d_shapes(g, views=3):
    """(name, (c_in, c_out, k, stride), (images, h, w)) of the twelve layers: the encoder on B * views images of four
    times the volume's H x W, the refinement net on B images of H x W."""
    out, h, w = [], 4 * g.n[1], 4 * g.n[2]
    for i, (cin, cout, k, s, _) in enumerate(model._ENCODER):
        out.append(("encoder %d" % i, (cin, cout, k, s), (g.batch * views, h, w)))
        h, w = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    for i, (cin, cout, k, s, _) in enumerate(model._REFINE):
        out.append(("refine %d" % i, (cin, cout, k, s), (g.batch, g.n[1], g.n[2])))
    return out


def conv2d_layers(g, dev, reps):
    for name, (cin, cout, k, s), (n, h, w) in conv2d_shapes(g):
        conv = torch.nn.Conv2d(cin, cout, k, stride=s, padding=k // 2, bias=False).to(dev)
        needs_gx = not name.startswith("encoder 0")   # the image needs no gradient
        x = torch.randn(n, cin, h, w, device=dev, requires_grad=needs_gx)
        with torch.no_grad():
            gy = torch.randn_like(tap_gemm.conv2d_hip_fwd(x, conv))

        def reset():
            x.grad = conv.weight.grad = None

        def taps():
            reset()
            tap_gemm.conv2d_hip_fwd(x, conv).backward(gy)

        def hip():
            reset()
            conv2d_train.conv2d_hip(x, conv).backward(gy)

        def alone(row):
            with torch.no_grad():
                xd, wd = x.detach(), conv.weight.detach()
                one_pass = round(hbm_ms((xd.numel() + gy.numel()) * 4), 4)
                row["forward_ms"] = ms(lambda: tap_gemm.conv2d_hip_fwd(xd, conv), reps)
                row["hip_gw_ms"] = ms(lambda: conv2d_train.conv2d_wgrad(xd, gy, k, s), reps)
                row["hip_gw_hbm_ms"] = one_pass
                if needs_gx:
                    row["hip_gx_ms"] = ms(lambda: conv2d_train.conv2d_dgrad(gy, wd, s, h, w), reps)
                    row["hip_gx_hbm_ms"] = one_pass
            row["tiles_slots"] = list(conv2d_train.wgrad_plan(n, cin, cout, h, w, k, s))
        yield Layer({"layer": name, "shape": [cin, cout, k, s], "x": [n, cin, h, w], "needs_gx": needs_gx,
                     "routed": (cin, cout, k, s) in conv2d_train.CONV2D_BWD_SHAPES},
                    (("taps", None, taps), ("hip", None, hip)), reset, alone)


FAMILIES = {
    "s1": Family("MVS_TRAIN_REGION_BWD", None, s1_layers),
    "s2": Family("MVS_TRAIN_S2_BWD", "GB", s2_layers),
    "t2": Family("MVS_TRAIN_T2_BWD", "GB", t2_layers),
    "deconv1": Family("MVS_TRAIN_DECONV1", "GB", deconv1_layers),
    "bn": Family("MVS_TRAIN_BN", "GB", bn_layers),
    "conv2d": Family("MVS_TRAIN_CONV2D_BWD", "MB", conv2d_layers),
}


def peak_memory(fn, reset, unit):
    reset()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated() if unit == "MB" else 0
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return round(peak / 1e6, 1) if unit == "MB" else round(peak / 1e9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(FAMILIES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dims", type=int, nargs=3, default=[192, 128, 160])
    a = ap.parse_args()
    fam = FAMILIES[a.family]
    assert fam.switch in train_switches.TABLE
    os.environ.pop("MVS_TRAIN_REGION_FWD", None)
    for layer in fam.layers(geometry(a), torch.device("cuda", 0), a.reps):
        row = layer.row
        for label, _, _ in layer.sides:
            row[label + "_ms"] = []
        for _ in range(a.runs):
            for label, value, fn in layer.sides:
                with switched(fam.switch, value):
                    row[label + "_ms"].append(ms(fn, a.reps))
        if fam.peak:
            for label, value, fn in layer.sides:
                with switched(fam.switch, value):
                    row["%s_peak_%s" % (label, "mem_GB" if fam.peak == "GB" else "MB")] = peak_memory(
                        fn, layer.reset, fam.peak)
        layer.reset()
        torch.cuda.empty_cache()
        layer.alone(row)
        print(json.dumps(row), flush=True)
        del layer, row
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
