"""The relations between the packed-mask entries (tests/mask_cross_inputs.py) on the GPU entries: the kernels of thirteen families
examine each other on one corpus -- re-framed by 1, 31, 63, 64 and 65 columns, under the eight isometries, and one entry's result as
the next one's input, the arrays as the first call returned them.  Every comparison is exact; tests/test_mask_cross_host.py shows
that the relations hold for the numpy statements and that they report subtly wrong entries."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import mask_cross_inputs as X  # noqa: E402

pytestmark = pytest.mark.gpu

OPS = X.GPU_OPS


@pytest.fixture(scope="module", autouse=True)
def entry_calls():
    yield
    print("\nmask_cross: %d entry calls: %s" % (sum(OPS.calls.values()), dict(OPS.calls)))


def _report(fails):
    for f in fails:
        print(f)
    return fails


@pytest.mark.parametrize("l", X.LEFTS)
def test_reframing_changes_nothing(l):
    for frame in X.frames_of(l):
        assert _report(X.rel_reframe(OPS, *frame)) == []


@pytest.mark.parametrize("code", X.CODES)
def test_isometries_commute(code):
    assert _report(X.rel_isometry(OPS, code)) == []


def test_c1_split_and_merge():
    assert _report(X.rel_split_merge(OPS)) == []


def test_c2_six_counts():
    assert _report(X.rel_counts(OPS)) == []
    assert _report(X.rel_counts(OPS, X.dirty(X.framed().img))) == []


def test_c3_loops_rasterised_back():
    assert _report(X.rel_loops(OPS)) == []


def test_c4_band_and_erosion():
    assert _report(X.rel_band(OPS)) == []


def test_c5_erosion_and_distance():
    assert _report(X.rel_erode_distance(OPS)) == []


def test_c6_duality():
    assert _report(X.rel_duality(OPS)) == []


def test_c7_hulls():
    assert _report(X.rel_hull(OPS)) == []


def test_c8_overlaps_and_algebra():
    assert _report(X.rel_overlaps_algebra(OPS)) == []
    assert _report(X.rel_overlaps_algebra(OPS, X.dirty(X.framed().img), X.dirty(X.in_image(X.other())))) == []


def test_c9_layers():
    assert _report(X.rel_layers(OPS)) == []


def test_c10_rle_round_trip():
    assert _report(X.rel_rle_round_trip(OPS)) == []


def test_c11_resize_by_two():
    assert _report(X.rel_resize(OPS)) == []


def test_d_producers_as_consumers():
    assert _report(X.rel_producers(OPS, X.NUMPY_OPS)) == []
