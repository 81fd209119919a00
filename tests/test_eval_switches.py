"""mvs_amd/eval_switches.py: the table of the eval-path MVS_* variables, held to what every variable meant before the
table existed (tests/golden/eval_switch_table.json, written on the parent commit by golden/make_eval_switch_table.py);
no environment read of a switch outside the tables, none under csrc/ outside common.h's env_int; on the GPU,
MVS_S2_LDS acting through ops.conv3d_region, and the fp32 region kernels that stayed against float64."""
import glob
import importlib.util
import json
import os
import re

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(_HERE)
PKG = os.path.join(REPO, "deep-multiview-depth-estimation_amd")
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def _generator():
    spec = importlib.util.spec_from_file_location("make_eval_switch_table",
                                                  os.path.join(_HERE, "golden", "make_eval_switch_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
with open(GEN.TABLE) as _f:
    GOLDEN = json.load(_f)


def _inline_now(state):
    """The five decisions that are inline in a larger function, as the code under test spells them."""
    from mvs_amd import eval_switches as es
    return {"model.deferred": state and es.cv_head(), "model.refine_glue": state and es.refine_glue(),
            "model.conv2d_words": state and es.conv2d_f16(), "regulariser.bw(eval)": state and es.region_split(),
            "regulariser.bw(train)": state and es.region_split()}


def test_fixture_is_from_the_parent_and_not_degenerate():
    assert len(GOLDEN["parent"]) == 40
    assert sorted(GOLDEN["table"]) == sorted(GEN.VARIABLES)
    for var in GEN.VARIABLES:
        assert sorted(GOLDEN["table"][var]) == sorted(GEN.key(v) for v in GEN.VALUES)
        # every variable changes some predicate for some value
        assert len(set(GOLDEN["table"][var].values())) > 1, var
    chunks = {r["MVSNet().pipeline_chunks"] for r in GOLDEN["records"]}
    assert {0, 1, 2, "ValueError: invalid literal for int() with base 10: 'junk'"} <= chunks
    # MVS_T2_LDS: 0 and 2 each move a slot count the default leaves alone (at the large and at the small region)
    t2 = GOLDEN["table"]["MVS_T2_LDS"]
    assert len({t2["<unset>"], t2["0"], t2["2"]}) == 3 and t2["1"] == t2["<unset>"]


@pytest.mark.parametrize("var", GEN.VARIABLES)
def test_every_predicate_answers_as_on_the_parent(var):
    """Each value of the variable (the others unset): CostVolumeReg.head_ok / _split_head_ok / _fp32_head_ok on
    stand-in tensors, the five inline decisions, MVSNet().pipeline_chunks and MVSConfig().arithmetic with their
    error messages, and the slot counts that follow MVS_T2_LDS."""
    for v in GEN.VALUES:
        with GEN.environment({var: v}):
            got = GEN.predicates(_inline_now)
        want = GOLDEN["records"][GOLDEN["table"][var][GEN.key(v)]]
        assert got == want, (var, v, {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]})


def test_the_table_names_the_twelve_variables():
    from mvs_amd import eval_switches as es
    assert tuple(sorted(es.TABLE)) == tuple(sorted(GEN.ALL_VARIABLES)) and len(es.TABLE) == 12
    rules = {"word", "is 1", "not 0", "starts 1", "atoi", "int", "library"}
    for row in es.TABLE.values():
        assert row.rule in rules and "DESIGN.md §" in row.doc, row.name
        assert not row.words or row.default in row.words, row.name
        assert ("read by the library" in row.doc) == (row.rule == "library"), row.name
    assert [n for n, r in es.TABLE.items() if r.rule == "library"] == ["MVS_CV_CSPLIT", "MVS_CONV2D_SPLIT"]
    with pytest.raises(KeyError):
        es.read("MVS_CV_CSPLIT")
    with pytest.raises(KeyError):
        es.on("MVS_T2_LDS")


def test_the_environment_is_read_on_every_call(monkeypatch):
    from mvs_amd import eval_switches as es
    monkeypatch.delenv("MVS_CV_HEAD", raising=False)
    monkeypatch.delenv("MVS_T2_LDS", raising=False)
    assert not es.cv_head() and es.t2_lds() == 1
    monkeypatch.setenv("MVS_CV_HEAD", "1")
    monkeypatch.setenv("MVS_T2_LDS", "2")
    assert es.cv_head() and es.t2_lds() == 2
    for value, taken in (("", 0), ("junk", 0), (" 2x", 2), ("-1", -1), ("+2", 2), ("0", 0)):   # C's atoi
        monkeypatch.setenv("MVS_T2_LDS", value)
        assert es.t2_lds() == taken, value
    for value, taken in (("1", True), ("10", True), ("0", False), ("", False), ("junk", False)):
        monkeypatch.setenv("MVS_S2_LDS", value)   # the first character, as the library tested it
        assert es.s2_lds() is taken, value


def test_t2_lds_becomes_flag_bits(monkeypatch):
    """ops passes MVS_T2_LDS as MVS_CONV_PER_LANE / MVS_CONV_T2_LDS, for a transposed convolution only, and
    per_lane wins."""
    from mvs_amd import _lib, ops
    for value, t2, t2_per_lane in ((None, 0, _lib.MVS_CONV_PER_LANE), ("1", 0, _lib.MVS_CONV_PER_LANE),
                                   ("0", _lib.MVS_CONV_PER_LANE, _lib.MVS_CONV_PER_LANE),
                                   ("2", _lib.MVS_CONV_T2_LDS, _lib.MVS_CONV_PER_LANE)):
        with GEN.environment({"MVS_T2_LDS": value}):
            assert ops._kernel_flags(ops.CONV_T2, False) == t2
            assert ops._kernel_flags(ops.CONV_T2, True) == t2_per_lane
            for mode in (ops.CONV_S1, ops.CONV_S2):
                assert ops._kernel_flags(mode, False) == 0
                assert ops._kernel_flags(mode, True) == _lib.MVS_CONV_PER_LANE
    assert _lib.MVS_CONV_T2_LDS == 512
    with open(os.path.join(REPO, "include", "mvs_cost_volume.h")) as f:
        assert "#define MVS_CONV_T2_LDS 512" in f.read()


def _package_sources():
    files = sorted(glob.glob(os.path.join(PKG, "mvs_amd", "**", "*.py"), recursive=True))
    assert len(files) > 10
    return files


def test_no_other_module_reads_an_mvs_variable():
    """A plain text search of the package sources: outside the two tables, _lib.py (MVS_LIB_PATH) and _build.py
    (MVS_OFFLOAD_ARCH) no line touches the environment and names an MVS_ variable, and regulariser.py, model.py
    and config.py do not touch it at all."""
    for path in _package_sources():
        name = os.path.basename(path)
        with open(path) as f:
            for n, line in enumerate(f, 1):
                reads = "environ" in line or "getenv" in line
                if name in ("regulariser.py", "model.py", "config.py"):
                    assert not reads and not re.match(r"\s*(import os\b|from os\b)", line), (path, n)
                if name not in ("eval_switches.py", "train_switches.py", "_lib.py", "_build.py"):
                    assert not (reads and "MVS_" in line), (path, n)


def test_the_library_reads_the_environment_only_through_env_int():
    """`getenv` appears under csrc/ only in common.h, once; env_int has the two callers the table lists."""
    files = sorted(glob.glob(os.path.join(PKG, "csrc", "*")))
    assert len(files) > 30
    calls = []
    for path in files:
        with open(path) as f:
            src = f.read()
        if os.path.basename(path) == "common.h":
            assert len(re.findall(r"\bgetenv\s*\(", src)) == 1
        else:
            assert "getenv" not in src, path
            calls += re.findall(r'\benv_int\("(\w+)"', src)
    assert sorted(calls) == ["MVS_CONV2D_SPLIT", "MVS_CV_CSPLIT"]


def test_readme_names_every_variable():
    with open(os.path.join(REPO, "README.md")) as f:
        readme = f.read()
    from mvs_amd import eval_switches
    for var, row in eval_switches.TABLE.items():
        assert "| `%s` |" % var in readme, var
        # the table's text is the row's doc line (without its "(DESIGN.md ...)" tail, a column of its own there)
        assert row.doc.rpartition(" (DESIGN.md ")[0] in readme, var


# ---- GPU ----
def _bit_differences(a, b):
    return int((a != b).sum().item())


@pytest.mark.gpu
def test_s2_lds_switch_acts_through_the_op(monkeypatch):
    """conv_1_0's shape (S2 32 -> 16 from the whole channel-quad volume, the smallest case of
    test_gpu_parity.py::test_region_s2_lds_kernel_matches_per_lane_and_float64: B = 2, 13 x 9 x 33) through
    ops.conv3d_region: with MVS_S2_LDS=1 and s2_lds=False the call equals the s2_lds=True call bit for bit; unset, the
    per_lane=True call; and the variable set after the first call of the process is followed by the next call."""
    from test_gpu_parity import _bn_params, _to_c4
    from mvs_amd.config import pad_outpad
    from mvs_amd.ops import CONV_S2, conv3d_region
    from mvs_amd.regions import _grow, _tconv_input_region, extent, origin
    b, n = 2, (13, 9, 33)
    pad, _ = pad_outpad(*n)
    h1 = _grow(_tconv_input_region(tuple((0, d - 1) for d in n), n, pad), n, 1)
    g = torch.Generator().manual_seed(57)
    x = _to_c4(torch.randn(b, 32, *n, generator=g).to(DEV))
    w27 = (torch.randn(27, 16, 32, generator=g) * 0.1).to(DEV)
    bn = [t.to(DEV) for t in _bn_params(16, g)]
    run = lambda **kw: conv3d_region(x, None, w27, CONV_S2, list(n), list(origin(h1)), list(extent(h1)), None, None,
                                     list(pad), *bn, in_c4=True, **kw)
    monkeypatch.delenv("MVS_S2_LDS", raising=False)
    with torch.no_grad():
        first = run()
        per_lane = run(per_lane=True)
        flagged = run(s2_lds=True)
        monkeypatch.setenv("MVS_S2_LDS", "1")      # after the first launches of the process
        by_switch = run()
        both = run(per_lane=True)                  # per_lane wins, as it did inside the library
        monkeypatch.delenv("MVS_S2_LDS")
        off_again = run()
    torch.cuda.synchronize()
    print("elements where the LDS-staged kernel's bits differ from the per-lane kernel's: %d of %d"
          % (_bit_differences(flagged, per_lane), flagged.numel()))
    assert torch.equal(first, per_lane) and torch.equal(off_again, per_lane) and torch.equal(both, per_lane)
    assert torch.equal(by_switch, flagged)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,cin,cout", [(0, 16, 16), (0, 32, 32), (0, 64, 64), (1, 32, 16), (1, 32, 32)])
def test_kept_fp32_region_kernels_match_float64(mode, cin, cout):
    """The fp32 region kernels that remain now that the LDS-staged stride-1 kernel and the four-row-block stride-2
    instantiations are gone: stride-1 C = 16 / 32 / 64 and stride-2 32 -> 16 / 32 from the channel-quad volume, B = 2,
    on the output region (5, 3, 17) at (1, 1, 1) of a (7, 5, 19) volume -- a partial tile in every dim -- against
    the zero-extended float64 reference and at the bound of tests/region_cases.py (check_fp32, what
    test_region_geometry.py holds these modes to)."""
    import torch.nn.functional as F
    from region_cases import cf, check_fp32, cl, conv_w27, extent, origin, sl, zero_ext
    from test_gpu_parity import _bn_params, _bn_relu, _to_c4
    from mvs_amd import ops
    from mvs_amd.config import pad_outpad
    b, n = 2, (7, 5, 19)
    reg, whole = tuple((1, d - 2) for d in n), tuple((0, d - 1) for d in n)
    assert tuple(extent(reg)) == (5, 3, 17)
    g = torch.Generator().manual_seed(100 * mode + cin + cout)
    wt = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.1
    bn = _bn_params(cout, g)
    bnd = [t.to(DEV) for t in bn]
    w27 = conv_w27(wt).to(DEV)
    if mode == 0:
        x = zero_ext(g, b, cin, n, whole)
        f = lambda xx, ww: _bn_relu(F.conv3d(xx, ww, padding=1), *(t.to(xx.dtype) for t in bn))[sl(reg)]
        args = (cl(x).to(DEV), None, w27, ops.CONV_S1, list(n), list(origin(reg)), list(extent(reg)),
                list(origin(whole)), list(extent(whole)), None)
        kw = {}
    else:
        pad = pad_outpad(*n)[0]
        x = torch.randn(b, cin, *n, generator=g).square()
        f = lambda xx, ww: _bn_relu(F.conv3d(xx, ww, stride=2, padding=pad), *(t.to(xx.dtype) for t in bn))[sl(reg)]
        args = (_to_c4(x.to(DEV)), None, w27, ops.CONV_S2, list(n), list(origin(reg)), list(extent(reg)), None, None,
                list(pad))
        kw = {"in_c4": True}
    with torch.no_grad():
        y = ops.conv3d_region(*args, *bnd, **kw)
        yp = ops.conv3d_region(*args, *bnd, per_lane=True, **kw)
    torch.cuda.synchronize()
    check_fp32(cf(y, False), f(x.double(), wt.double()), f(x, wt), "mode %d %d -> %d" % (mode, cin, cout))
    assert torch.equal(y, yp)
