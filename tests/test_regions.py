"""CPU: the live-region plan (mvs_amd.regions) -- live_regions against the hand-chained
_tconv_input_region, origin / extent as the C ABI's lists, and the names mvs_amd.model re-exports."""
import pytest

from mvs_amd import bn_sums, model, regions, regulariser, streams
from mvs_amd.config import pad_outpad

# even and odd extents, extent 1, and volumes so small that the chain stops shrinking (C3 == C2 == B)
SHAPES = [(8, 12, 16), (7, 9, 11), (2, 3, 4), (3, 1, 5), (13, 10, 17)]


def _chain(n):
    pad = pad_outpad(*n)[0]
    full = tuple((0, d - 1) for d in n)
    B = regions._tconv_input_region(full, n, pad)
    C2 = regions._tconv_input_region(B, n, pad)
    C3 = regions._tconv_input_region(C2, n, pad)
    return full, B, C2, C3


@pytest.mark.parametrize("n", SHAPES)
def test_live_regions_equal_hand_chain(n):
    got = regions.live_regions(n, pad_outpad(*n)[0])
    assert got == _chain(n)
    full, B, C2, C3 = got
    assert full == tuple((0, d - 1) for d in n)
    for outer, inner in ((full, B), (B, C2), (C2, C3)):   # nested, never empty
        assert all(olo <= lo <= hi <= ohi for (olo, ohi), (lo, hi) in zip(outer, inner))


@pytest.mark.parametrize("n", SHAPES)
def test_origin_extent_round_trip(n):
    for reg in _chain(n):
        org, ext = regions.origin(reg), regions.extent(reg)
        assert isinstance(org, list) and isinstance(ext, list)
        assert org == [lo for lo, _ in reg] and ext == [hi - lo + 1 for lo, hi in reg]
        assert tuple((o, o + e - 1) for o, e in zip(org, ext)) == reg


@pytest.mark.parametrize("home,names", [
    (regions, ("_grow", "_tconv_input_region", "_crop_pad", "_conv_s2_region", "_conv_s1_region", "_tconv_region")),
    (regulariser, ("_bn_eval", "CostVolumeReg")),
    (bn_sums, ("_bn_train", "_bn_constant", "_border_class_sums", "_border_tables_u")),
    (streams, ("_side_stream", "_LANE")),
])
def test_model_reexports_are_the_same_objects(home, names):
    for name in names:
        assert getattr(model, name) is getattr(home, name), name
