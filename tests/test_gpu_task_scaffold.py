"""The one timing span of the host-array entries (csrc/mnc_internal.h: CallTimer, TimedSpan) behind each of its four switches:
with the switch off a call keeps nothing, with it on the call's launches leave a figure above zero -- for the polygons also the
sizes-only call, which launches the rasteriser.  One call each on the smallest input that launches anything; no two times are
compared."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_overlap_inputs  # noqa: E402,F401  (sets up the import paths)
from mnc_amd import _lib, boundary, coco_eval, components, polygons  # noqa: E402
from mnc_amd.masks import PackedMasks  # noqa: E402

pytestmark = pytest.mark.gpu


def boundary_call():
    """Two instances in a 70 x 5 image at d = 1."""
    pm = PackedMasks.from_dense([[0, 0, 69, 4], [3, 1, 40, 3]], [np.ones((5, 70), bool), np.ones((3, 38), bool)])
    room = np.zeros(5 * 2 + 3, np.uint64)
    return lambda: boundary.boundary_call(pm, 5, 70, 1, room)


def components_call():
    """One 65 x 2 mask with two runs."""
    m = np.zeros((2, 65), bool)
    m[0, :3] = m[0, 62:] = True
    pm = PackedMasks.from_dense([[0, 0, 64, 1]], [m])
    return lambda: components.components(pm, 8)


def polygons_calls():
    """One triangle in a 70 x 5 image: the call with room, and the sizes-only call."""
    checked, H, W = polygons._check_segs("test", [[[1.0, 0.5, 68.0, 0.5, 30.0, 4.5]]], 5, 70)
    xy, vert_ptr, poly_ptr = polygons._flatten(checked)
    room = np.zeros(5 * 2, np.uint64)
    return (lambda: polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, room),
            lambda: polygons.masks_from_polygons_call(xy, vert_ptr, poly_ptr, H, W, None))


def accumulate_call():
    """N = 3, Gn = 2, K = T = A = M = R = 1."""
    flat = {"dt_class_idx": np.zeros(3, np.int32), "dt_score": np.array([0.9, 0.5, 0.7], np.float32),
            "dt_rank": np.arange(3, dtype=np.int32), "dt_flags": np.array([[[1, 0, 1]]], np.uint8),
            "gt_class_idx": np.zeros(2, np.int32), "gt_ignore": np.zeros((1, 2), np.uint8)}
    return lambda: coco_eval.accumulate_flat(flat, 1, [100], [0.5])


CALLS = {
    "mnc_mask_boundary_timing": lambda: (boundary_call(),),
    "mnc_mask_components_timing": lambda: (components_call(),),
    "mnc_mask_poly_timing": polygons_calls,
    "mnc_coco_accum_timing": lambda: (accumulate_call(),),
}


@pytest.mark.parametrize("entry", list(CALLS))
def test_a_call_keeps_its_launches_time_only_while_the_switch_is_on(entry):
    calls = CALLS[entry]()
    try:
        _lib.timing(entry, True)                                 # forgets whatever was kept
        assert _lib.timing(entry, False) == -1.0
        calls[0]()
        assert _lib.timing(entry, False) == -1.0                 # off: the call kept nothing
        for call in calls:                                       # (polygons: the sizes-only call as well)
            _lib.timing(entry, True)
            call()
            assert _lib.timing(entry, False) > 0.0
    finally:
        _lib.timing(entry, False)
