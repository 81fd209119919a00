"""The region convolutions (csrc/conv3d_region.hip, csrc/conv3d_region_split.hip) against bit pins of the
commit before their shared pieces moved into csrc/region_conv.h (tests/golden/region_conv_pins.json, written
by tests/golden/make_region_pins.py ON THAT COMMIT, named in the file): SHA-256 of every case's output bytes,
output bound words and float64 sum slots, recomputed with the code under test.  The cases
(make_region_pins.cases): the split per-lane, S1-LDS and T2-LDS kernels in both layouts with x2, folded
input BN, output addend and store box + sums, at volumes whose regions start off 0 and end inside tiles;
the fp32 kernels from every input layout, and the fused head's in-place slab stores.
"""
import json

import pytest

import make_region_pins as pins


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
def test_region_conv_bits_as_pinned(key, pinned, monkeypatch):
    assert pins.run_case(key, monkeypatch.setenv) == pinned[key], key
