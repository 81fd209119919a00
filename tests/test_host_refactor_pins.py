"""The host layers (mvs_amd/ops.py wrappers, csrc/capi.hip weight splits) against records of the commit
before their shared helpers were folded out (tests/golden/host_pins.json, written by
tests/golden/make_host_pins.py ON THAT COMMIT, named in the file): the same record functions run on the
code under test must give the same values.  No GPU: the weight splits run on the host, the rest is op
metadata.
"""
import json

import pytest

import make_host_pins as pins


@pytest.fixture(scope="module")
def pinned():
    with open(pins.PINS) as f:
        doc = json.load(f)
    assert len(doc["parent"]) == 40
    return doc


def test_fragment_bytes_and_exponents(pinned):
    """Every weight-split entry point at every shape the model uses (conv_0_0 8x32, conv_1_0 16x32,
    CONV2D_SPLIT_SHAPES, the region weights and train's 112x32 concatenation) x (hash weights, all-zero ->
    exponent 0, max an exact power of two, max 1e-38 -> the +120 clamp, max 1e30 -> a negative exponent,
    one NaN -> status -1): fragment SHA-256, length, exponent and status as pinned."""
    want = pinned["fragments"]
    assert len(want) == len(pins.fragment_targets()) * len(pins.CASES)
    got = pins.fragment_records()
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
    for key, rec in want.items():   # the cases are the ones named above, not just equal to themselves
        case = key.rsplit("/", 1)[1]
        if case == "nan":
            assert rec == {"status": -1}, key
        else:
            assert rec["status"] == 0 and {"zero": rec["exp"] == 0, "tiny": rec["exp"] == 120,
                                           "huge": rec["exp"] < 0}.get(case, True), key


def test_op_schemas(pinned):
    got = pins.schema_records()
    assert sorted(got) == sorted(pinned["schemas"])
    for name, schema in pinned["schemas"].items():
        assert got[name] == schema, name


def test_fake_kernel_shapes_and_dtypes(pinned):
    """The six cost-volume ops and cost_volume_head (with and without a stored box) under FakeTensorMode at
    (B, V, C, h, w, D) = (2, 3, 32, 16, 20, 12)."""
    got = pins.fake_records()
    assert sorted(got) == sorted(pinned["fakes"]) and len(got) == 8
    for name, outs in pinned["fakes"].items():
        assert got[name] == outs, name
