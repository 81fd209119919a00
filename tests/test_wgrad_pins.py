"""The tap-row weight-gradient kernels (csrc/conv3d_region_wgrad.hip, csrc/conv3d_s2_wgrad.hip,
csrc/conv3d_t2_wgrad.hip, csrc/deconv3d_region_bwd.hip) against bit pins of the commit before their shared plan
moved into csrc/wgrad_taprow.h (tests/golden/wgrad_pins.json, written by tests/golden/make_wgrad_pins.py ON THAT
COMMIT, named in the file): SHA-256 of dw's bytes, recomputed through the mvs_amd.ops wrappers with the code under
test.  The cases (make_wgrad_pins.cases): every kernel instantiation at a single-pass shape with partly filled
tiles and skipped rows, and at the smallest multi-pass shape of the float64 tests.
"""
import json

import pytest

import make_wgrad_pins as pins


@pytest.fixture(scope="module")
def pinned():
    with open(pins.PINS) as f:
        doc = json.load(f)
    assert len(doc["parent"]) == 40
    return doc["cases"]


@pytest.mark.gpu
def test_every_case_is_pinned(pinned):
    assert sorted(pinned) == sorted(pins.cases())


@pytest.mark.gpu
@pytest.mark.parametrize("key", sorted(pins.cases()))
def test_wgrad_bits_as_pinned(key, pinned):
    assert pins.run_case(key) == pinned[key], key
