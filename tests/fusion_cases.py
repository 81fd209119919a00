"""The plane scenes of the depth-map filtering tests, each built once with its float64 restatement (fusion_ref) and
shared, unchanged, by test_fusion_abi.py (the restatement's own margins, no GPU) and test_fusion_gpu.py."""
import functools

import numpy as np

import fusion_ref

# (h, w, N, S): 1x1 .. one 128x160; N in {1, 2, 5}, S in {1, 4, 10}; N h w = 175, 1485 and 3400 are no multiples of 64
SCENES = ((1, 1, 1, 1), (2, 2, 2, 1), (5, 7, 2, 4), (5, 7, 5, 10), (9, 33, 5, 4), (17, 40, 5, 10), (128, 160, 5, 4),
          (128, 160, 2, 1))
# the scenes on which the restatement must reach the full count on a majority of the interior pixels
FULL_COUNT = ((17, 40, 5, 10), (128, 160, 5, 4), (128, 160, 2, 1))
FULL_COUNT_SHARE = 0.5


def pair_lists(n_views, n_slots):
    """Ragged source lists for N views and at most S slots: -1 holes, a slot naming its own view, a view without
    sources, repeated sources where S exceeds the other views."""
    if n_views == 1:
        return [[0] if n_slots == 1 else [-1, 0]]
    if n_views == 2:
        return [[1], [0]] if n_slots == 1 else [[-1, 1, 1], [0, 1, -1, 0]]
    others = lambda i: [v for v in range(n_views) if v != i]
    if n_slots == 4:
        return [others(0), [0, 2], [3, 2, -1, 1], [4], []]                     # (view 2 names itself; view 4: none)
    rows = [(others(i) * 3)[:n_slots] for i in range(n_views)]
    rows[1] = rows[1][:7]
    rows[2][4] = 2
    rows[3] = [-1, -1] + others(3)
    return rows


@functools.lru_cache(maxsize=None)
def scene(h, w, n_views, n_slots):
    """dict: K, R, T, depth (fp32 arrays), pairs (the ragged list), table [N, S], and the restatement's count, avg,
    near at the default thresholds."""
    K, R, T = fusion_ref.arc_cameras(n_views, h, w)
    depth = fusion_ref.plane_depths(K, R, T, h, w)
    pairs = pair_lists(n_views, n_slots)
    table = fusion_ref.pad_pairs(pairs)
    assert table.shape == (n_views, n_slots), table.shape
    count, avg, near = fusion_ref.consistency(depth, K, R, T, table)
    for a in (K, R, T, depth, table, count, avg, near):
        a.setflags(write=False)
    return {"K": K, "R": R, "T": T, "depth": depth, "pairs": pairs, "table": table, "count": count, "avg": avg,
            "near": near}


def interior(h, w):
    """The pixels at least an eighth of the map away from its border."""
    m = np.zeros((h, w), bool)
    m[h // 8:h - h // 8, w // 8:w - w // 8] = True
    return m


def full_count_share(sc):
    """The share of interior pixels, over the views that have a source, on which the restatement counts every
    non-empty slot."""
    slots = fusion_ref.non_empty_slots(sc["table"])
    h, w = sc["depth"].shape[2:]
    inner = interior(h, w)
    views = [n for n in range(len(slots)) if slots[n] > 0]
    full = np.stack([sc["count"][n, 0][inner] == slots[n] for n in views])
    return float(full.mean())
