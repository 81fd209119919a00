"""mvs_amd/train_switches.py: the table of MVS_TRAIN_* variables, held to what every variable meant before the table
existed (tests/golden/train_switch_table.json, written on the parent commit by golden/make_train_switch_table.py),
the per-family routing functions of region_train held to the parent's pair of decisions, and on the GPU one
regulariser + refinement step under the "all_hip" preset."""
import copy
import glob
import importlib.util
import json
import os

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def _generator():
    spec = importlib.util.spec_from_file_location("make_train_switch_table",
                                                  os.path.join(_HERE, "golden", "make_train_switch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
with open(GEN.TABLE) as _f:
    GOLDEN = json.load(_f)


def _run_stack_now():
    from mvs_amd import model
    return list(model.conv2d_train_backends())


def test_fixture_is_from_the_parent_and_not_degenerate():
    assert len(GOLDEN["parent"]) == 40
    assert sorted(GOLDEN["table"]) == sorted(GEN.VARIABLES)
    for var in GEN.VARIABLES:
        assert sorted(GOLDEN["table"][var]) == sorted(GEN.key(v) for v in GEN.VALUES)
        # every variable changes some predicate for some value
        assert len({json.dumps(GOLDEN["table"][var][GEN.key(v)], sort_keys=True) for v in GEN.VALUES}) > 1, var
    assert any(str(r["model.conv2d_bwd_mode"]).startswith("ValueError: MVS_TRAIN_CONV2D_BWD must be")
               for r in GOLDEN["records"])
    for family, codes in (("s2", "-0123"), ("s1", "-23"), ("tconv", "-23")):
        assert set("".join(GOLDEN["routes"][family].values())) == set(codes), family


@pytest.mark.parametrize("var", GEN.VARIABLES)
def test_every_predicate_answers_as_on_the_parent(var):
    """Each value of the variable (the others unset) x tensor on / off the GPU, grad mode on / off, fp16: every
    public predicate, conv2d_bwd_mode's error message included, and model.conv2d_train_backends against the two
    reads that were inline in _run_stack."""
    for v in GEN.VALUES:
        for name, is_cuda, dtype, grad in GEN.CONTEXTS:
            with GEN.environment({var: v}), torch.set_grad_enabled(grad):
                got = GEN.predicates(is_cuda, dtype, _run_stack_now)
            want = GOLDEN["records"][GOLDEN["table"][var][GEN.key(v)][name]]
            assert got == want, (var, v, name, {k: (got[k], want[k]) for k in want if got.get(k) != want[k]})


def _with_taps(route):
    """The routing functions are asked inside regions.py's own _taps(x) branch."""
    from mvs_amd.regions import _taps

    def decide(x, *a):
        return route(x, *a) if _taps(x) else None
    return decide


@pytest.mark.parametrize("family", ["s2", "s1", "tconv"])
def test_routes_are_the_parents_two_decisions_composed(family):
    """region_train.s2_route / s1_route / tconv_route over (MVS_TRAIN_REGION_FWD x the family's backward switches)
    x (whole, splits, channels, dims is None) x (GPU / CPU, grad / no_grad): None or the (hip_fwd, hip_bwd) pair,
    equal to the parent's regions.py condition followed by its s2_box / _S1Valid / t2_box / d1_applies decision."""
    from mvs_amd import region_train
    route = {"s2": region_train.s2_route, "s1": region_train.s1_route, "tconv": region_train.tconv_route}[family]
    got = GEN.route_rows(family, _with_taps(route))
    want = GOLDEN["routes"][family]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, dict(list(wrong.items())[:5])


def test_direct_box_calls_decide_as_on_the_parent(monkeypatch):
    """s2_box / s1_valid / t2_box called without a route (as the GPU tests call them) pick the parent's backends:
    neither switch keeps the HIP stride-2 forward; MVS_TRAIN_S2_BWD alone takes the tap-GEMM forward."""
    from mvs_amd import region_train as rt
    seen = []
    for box in (rt._S2Box, rt._S1Valid, rt._T2Box):
        monkeypatch.setattr(box, "apply", staticmethod(lambda *a: seen.append(a)))
    x, w1 = GEN.Stub(True, torch.float32, (2, 32, 9, 9, 9)), GEN.Stub(False, torch.float32, (32, 32, 3, 3, 3))
    for fwd in GEN.VALUES:
        for bwd in GEN.FEW + ("s1",):
            env = {"MVS_TRAIN_REGION_FWD": fwd, "MVS_TRAIN_S2_BWD": bwd, "MVS_TRAIN_T2_BWD": bwd,
                   "MVS_TRAIN_REGION_BWD": bwd}
            with GEN.environment(env):
                for splits in (rt.S2_SPLITS, (16,)):
                    rt.s2_box(x, None, None, None, None, splits)
                    hip_bwd = rt.s2_bwd_enabled(x) and tuple(splits) == rt.S2_SPLITS
                    assert seen.pop()[-2:] == (rt.enabled(x, "s2") or not rt.s2_bwd_enabled(x), hip_bwd)
                rt.s1_valid(x, w1)
                assert seen.pop()[-1] == rt.bwd_enabled("s1", 32)
                for pair in ((64, 32), (16, 8)):
                    w = GEN.Stub(False, torch.float32, pair + (3, 3, 3))
                    rt.t2_box(x, w, None, None, None, None, None)
                    assert seen.pop()[-1] == (rt.t2_bwd_enabled(x) and pair in rt.T2_SHAPES)
    with GEN.environment({}):
        rt.s2_box(x, None, None, None, None, rt.S2_SPLITS)
        assert seen.pop()[-2:] == (True, False)
    with GEN.environment({"MVS_TRAIN_S2_BWD": "hip"}):
        rt.s2_box(x, None, None, None, None, rt.S2_SPLITS)
        assert seen.pop()[-2:] == (False, True)


def test_the_table_names_exactly_the_eleven_variables():
    from mvs_amd import train_switches
    assert tuple(train_switches.TABLE) == GEN.VARIABLES and len(GEN.VARIABLES) == 11
    for row in train_switches.TABLE.values():
        assert row.default in row.words or all(k in row.kinds for k in row.default.split(",")), row.name
        assert "DESIGN.md §" in row.doc, row.name


def test_no_other_module_reads_a_training_variable():
    """A plain text search of the package sources: outside train_switches.py no line both touches the environment
    and names a MVS_TRAIN_ variable."""
    pkg = os.path.join(REPO, "deep-multiview-depth-estimation_amd", "mvs_amd")
    files = sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True))
    assert len(files) > 10
    for path in files:
        if os.path.basename(path) == "train_switches.py":
            continue
        with open(path) as f:
            for n, line in enumerate(f, 1):
                assert not ("MVS_TRAIN_" in line and ("environ" in line or "getenv" in line)), (path, n)


def test_readme_names_every_variable():
    with open(os.path.join(REPO, "README.md")) as f:
        readme = f.read()
    from mvs_amd import train_switches
    for var in GEN.VARIABLES:
        assert "| `%s` |" % var in readme, var
        # the table's text is the row's doc line (without its "(DESIGN.md ...)" tail, a column of its own there)
        assert train_switches.TABLE[var].doc.rpartition(" (DESIGN.md ")[0] in readme, var


def test_presets():
    from mvs_amd import train_switches as ts
    assert ts.PRESETS["default"] == {}
    assert ts.PRESETS["all_hip"] == {"MVS_TRAIN_REGION_BWD": "hip", "MVS_TRAIN_S2_BWD": "hip",
                                     "MVS_TRAIN_T2_BWD": "hip", "MVS_TRAIN_DECONV1": "hip", "MVS_TRAIN_BN": "hip",
                                     "MVS_TRAIN_CONV2D_BWD": "hip"}
    for name, value in ts.PRESETS["all_hip"].items():
        assert ts.accepts(name, value), (name, value)
        with GEN.environment({name: value}):
            assert ts.read(name) == value
    assert not ts.accepts("MVS_TRAIN_BN", "taps") and ts.accepts("MVS_TRAIN_REGION_FWD", "s2,t2")
    assert ts.parse_assignment("all_hip") == ts.PRESETS["all_hip"] and ts.parse_assignment("default") == {}
    assert ts.parse_assignment("MVS_TRAIN_REGION_FWD=s1,t2,MVS_TRAIN_BN=hip") == {"MVS_TRAIN_REGION_FWD": "s1,t2",
                                                                                 "MVS_TRAIN_BN": "hip"}
    assert ts.parse_assignment("MVS_TRAIN_LIVE=0") == {"MVS_TRAIN_LIVE": "0"}
    for bad in ("MVS_TRAIN_NOPE=1", "fast"):
        with pytest.raises(ValueError):
            ts.parse_assignment(bad)


def test_the_environment_is_read_on_every_call(monkeypatch):
    from mvs_amd import train_switches as ts
    monkeypatch.delenv("MVS_TRAIN_BN", raising=False)
    assert ts.read("MVS_TRAIN_BN") == "torch"
    monkeypatch.setenv("MVS_TRAIN_BN", "hip")
    assert ts.read("MVS_TRAIN_BN") == "hip"
    monkeypatch.setenv("MVS_TRAIN_BN", "")
    assert ts.read("MVS_TRAIN_BN") == ""            # empty is no word here ...
    monkeypatch.setenv("MVS_TRAIN_CONV2D_BWD", "")
    assert ts.read("MVS_TRAIN_CONV2D_BWD") == "taps"   # ... and the default there


# (module attribute, function) of every HIP gradient op the "all_hip" preset brings in, by family
_GRADIENT_OPS = {
    "s1": (("ops", "conv3d_region_wgrad"),),
    "s2": (("ops", "conv3d_s2_region_wgrad"), ("ops", "conv3d_s2_region_dgrad")),
    "t2": (("ops", "conv3d_t2_region_wgrad"), ("ops", "conv3d_t2_region_dgrad")),
    "deconv1": (("ops", "deconv3d_k3s2_wgrad"), ("ops", "deconv3d_k3s2_dgrad")),
    "bn": (("bn_train", "bn_relu_train"),),
    "conv2d": (("conv2d_train", "conv2d_wgrad"), ("conv2d_train", "conv2d_dgrad")),
}


@pytest.mark.gpu
def test_all_hip_preset_runs_every_family_and_matches_float64(monkeypatch):
    """One regulariser forward + backward (test_bn_train_routing.py's chain: B = 2, volume (20, 32, 40), loss
    sum(P * Wr)) and one refinement-stack forward + backward (test_conv2d_train_bwd.py's chain: 2 images of 36 x 44)
    under PRESETS["all_hip"], then under PRESETS["default"].  Every HIP gradient op of the six families is called at
    least once under the preset and never under the default.  Every parameter gradient, the input gradients and every
    BN running statistic: relative L2 to float64 CPU autograd <= 2 x the CPU fp32 path's own + 1e-5 -- the bound of
    test_bn_train_routing.py::test_regulariser_chain_with_hip_bn (and of test_conv2d_train_bwd.py::test_chain),
    whose references are shared -- for both runs, so the preset's gradients sit as close to float64 as the
    default's."""
    from mvs_amd import train_switches
    from mvs_amd.model import _run_stack
    from test_bn_train_routing import _chain_reference as reg_reference, _rel, _step
    from test_conv2d_train_bwd import _chain_reference as stack_reference
    seen = {}

    def counted(mod, name):
        orig = getattr(mod, name)

        def f(*a, **k):
            seen[name] = seen.get(name, 0) + 1
            return orig(*a, **k)
        return f
    for family in _GRADIENT_OPS.values():
        for mod_name, name in family:
            mod = importlib.import_module("mvs_amd." + mod_name)   # (conv2d_train registers its ops on import)
            monkeypatch.setattr(mod, name, counted(mod, name))
    reg, cv, wr, pc, pd, cvg_c, cvg_d, bc, bd = reg_reference()
    seq, x, swr, g64, g32 = stack_reference("refine")
    for preset in ("all_hip", "default"):
        for name in train_switches.TABLE:
            monkeypatch.delenv(name, raising=False)
        for name, value in train_switches.PRESETS[preset].items():
            monkeypatch.setenv(name, value)
        seen.clear()
        _, cvg_g, pg, bg = _step(copy.deepcopy(reg).to(DEV), cv.to(DEV), wr.to(DEV), lambda m, t: m(t))
        net = copy.deepcopy(seq).to(DEV)
        xg = x.to(DEV).requires_grad_(True)
        (_run_stack(net, xg) * swr.to(DEV)).sum().backward()
        if preset == "all_hip":
            missing = [n for fam in _GRADIENT_OPS.values() for _, n in fam if not seen.get(n)]
            assert not missing, (missing, seen)
        else:
            assert seen == {}, seen
        errs = {"reg." + k: (_rel(pg[k].cpu(), pd[k]), _rel(pc[k], pd[k])) for k in sorted(pd) if pd[k] is not None}
        errs["reg.cost_volume"] = (_rel(cvg_g.cpu(), cvg_d), _rel(cvg_c, cvg_d))
        for k in sorted(bd):
            if k.endswith("num_batches_tracked"):
                assert torch.equal(bg[k].cpu(), bd[k]), k
            else:
                errs["reg." + k] = (_rel(bg[k].cpu(), bd[k]), _rel(bc[k], bd[k]))
        got = {k: p.grad for k, p in net.named_parameters()}
        got["input"] = xg.grad
        for k in sorted(g64):
            errs["refine." + k] = (_rel(got[k].cpu(), g64[k]), _rel(g32[k], g64[k]))
        assert {"reg.BN_0.weight", "reg.conv_3_1.weight", "reg.deconv_1_0.weight", "reg.deconv_3_0.weight",
                "reg.conv_1_0.weight", "reg.BN_3.running_var", "refine.0.weight", "refine.input"} <= set(errs)
        worst = max(errs, key=lambda k: errs[k][0] / (2.0 * errs[k][1] + 1e-5))
        print("%s: worst tensor %s: GPU %.3g, CPU fp32 %.3g, bound %.3g"
              % (preset, worst, errs[worst][0], errs[worst][1], 2.0 * errs[worst][1] + 1e-5))
        for k, (e_g, e_c) in errs.items():
            assert e_g <= 2.0 * e_c + 1e-5, "%s, %s: GPU %.3g from float64, CPU fp32 %.3g" % (preset, k, e_g, e_c)
