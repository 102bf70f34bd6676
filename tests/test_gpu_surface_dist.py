"""Surface distances between packed instance masks on the GPU (csrc/mask_surface.hip: mnc_mask_surface, mnc_mask_surface_stats,
mnc_mask_surface_dist and the Python surfaces over them) against the numpy statements (mnc_amd.surface.surface_numpy,
surface_stats_numpy and surface_distances_numpy, which tests/test_surface_dist_host.py pins to scipy and to closed forms) and
against the existing kernels (erode, dilate, the set algebra).  Every comparison is exact, field by field, dtype and shape
included, and every device call is made twice: the bytes are equal.  The sets are those of tests/surface_dist_inputs.py: the
smallest at which a kernel can go wrong."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import surface_dist_inputs as SI  # noqa: E402
from mnc_amd import _lib  # noqa: E402
from mnc_amd import surface as SF  # noqa: E402
from mnc_amd.masks import PackedMasks, _set_args  # noqa: E402
from transform import mask_transform as MT  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID = 1
CANARY32 = 0x55555555
CANARY64 = 0x5555555555555555


def _bytes(t):
    return [a.tobytes() for a in t]


def _stats(a, b, pairs, want, tau2=SI.TAU2):
    """surface_stats twice, against the statement's result."""
    first = SF.surface_stats(a, b, pairs, tau2)
    assert SI.same_fields(first, want)
    assert _bytes(SF.surface_stats(a, b, pairs, tau2)) == _bytes(first)
    return first


def _dist(a, b, pairs, want):
    first = SF.surface_distances(a, b, pairs)
    assert SI.same_fields(first, want)
    assert _bytes(SF.surface_distances(a, b, pairs)) == _bytes(first)
    return first


def _surface(pm):
    first = SF.surface(pm)
    assert SI.same_set(first, SF.surface_numpy(pm))
    assert _bytes(SF.surface(pm).arrays().values()) == _bytes(first.arrays().values())
    return first


def _case(name):
    a, b, pairs = SI.get(name)
    return _stats(a, b, pairs, SI.stats_ref(name)), _dist(a, b, pairs, SI.dist_ref(name))


# ---- word edges ----

def test_word_edge_widths_heights_and_starts_with_dirty_padding():
    """Widths 1, 63, 64, 65, 129 by heights 1, 2, 65 at x1 = 0, 1, 63 modulo 64, every instance against the next and against
    itself; the copy with clean padding gives the same bytes."""
    pm, _, pairs = SI.get("word_edges")
    w, h = pm.bounds[:, 2] - pm.bounds[:, 0] + 1, pm.bounds[:, 3] - pm.bounds[:, 1] + 1
    assert set(w.tolist()) == set(SI.WIDTHS) and set(h.tolist()) == set(SI.HEIGHTS) and set((pm.bounds[:, 0] % 64).tolist()) == set(SI.STARTS)
    clean = SI.word_edges_set(dirty=False)
    assert not np.array_equal(clean.bits, pm.bits)                     # the padding bits of the set are ones
    st, d = _case("word_edges")
    assert _bytes(SF.surface_stats(clean, clean, pairs, SI.TAU2)) == _bytes(st)
    assert _bytes(SF.surface_distances(clean, clean, pairs)) == _bytes(d)
    own = st.max_d2[0::2]                                              # (i, i): a surface against itself
    assert not own.any() and np.array_equal(st.within[0::2, :, 0], st.count[0::2]) and st.max_d2[1::2].any()
    s = _surface(pm)
    assert _bytes(SF.surface(clean).arrays().values()) == _bytes(s.arrays().values())


# ---- the walk ----

def test_single_pixels_in_the_eight_sectors_around_a_3x3_and_inside_it():
    st, d = _case("sectors")
    a, b, _ = SI.get("sectors")
    for k in range(len(a)):
        x, y = (int(v) for v in a.bounds[k][:2])
        dx, dy = max(10 - x, 0, x - 12), max(10 - y, 0, y - 12)
        assert st.max_d2[k, 0] == (dx * dx + dy * dy if dx or dy else 1)            # the centre is 1 from the ring of 8
        assert d.slot(k, 1).max() == max((x - qx) ** 2 + (y - qy) ** 2 for qx in (10, 12) for qy in (10, 12))
    assert st.count[:, 1].tolist() == [8] * 9


@pytest.mark.parametrize("name", ["far", "empty_rows", "ring"])
def test_far_surface_pixels_empty_rows_and_a_dot_in_a_ring(name):
    st, d = _case(name)
    if name == "far":
        assert st.max_d2[0, 0] == 5 ** 2 + 2 ** 2 and st.max_d2[1, 0] == 61 ** 2 + 2 ** 2      # (-5, 1) -> (0, 3); (260, 4) -> (199, 2)
        assert st.max_d2[3, 0] == min(99 ** 2, 100 ** 2 + 1)                                  # (100, 2) -> (199, 2), not (0, 3)
    if name == "ring":
        assert d.slot(0, 1).tolist() == [49] and st.max_d2[0, 0] == 144 and d.slot(0, 0).min() == 49


def test_equal_maxima_in_other_words_waves_and_workgroups_go_to_the_lowest_y_x():
    st, d = _case("ties")
    assert st.max_d2.tolist() == [[SI.TIE_D2] * 2]
    assert tuple(st.argmax[0, 0]) == SI.TIE_SPOTS[0] and tuple(st.argmax[0, 1]) == (SI.TIE_SPOTS[0][0] + 3, SI.TIE_SPOTS[0][1] + 4)
    assert (d.slot(0, 0) == SI.TIE_D2).sum() == len(SI.TIE_SPOTS) == (d.slot(0, 1) == SI.TIE_D2).sum()
    assert st.count[0, 0] > len(SI.TIE_SPOTS) and st.sum_d2.tolist() == [[SI.TIE_D2 * len(SI.TIE_SPOTS)] * 2]


def test_a_source_of_sixteen_workgroups_against_a_sparse_destination():
    st, d = _case("large")
    a = SI.get("large")[0]
    assert a.size(0) == (200, 300) and st.count[0, 0] > 20000 and st.count[0, 1] == 20
    assert st.max_d2[0, 0] > 40 ** 2                                   # deep walks


def test_130_small_instances_all_16900_pairs():
    a = SI.get("many130")[0]
    assert len(a) == 130
    st, d = _case("many130")
    assert st.count.shape == (16900, 2) and d.ptr.shape == (33801,) and d.ptr[-1] == 2 * 130 * st.count[:130, 1].sum()


# ---- the ends ----

def test_bounds_at_the_ends_of_the_span():
    for reach, want in ((16000, 2 * 32000 ** 2), (16383, 2 * 32766 ** 2)):
        a, b = SI.extreme_sets(reach)
        st = _stats(a, b, None, SF.surface_stats_numpy(a, b, None, SI.TAU2))
        assert st.max_d2.tolist() == [[want, want]] and want < 2 ** 31 and st.within[0, :, -1].tolist() == [1, 1]
        assert st.argmax.tolist() == [[[-reach, -reach], [reach, reach]]]
        assert _dist(a, b, None, SF.surface_distances_numpy(a, b)).d2.tolist() == [want, want]
    a, b = SI.extreme_sets(16384)
    with pytest.raises(ValueError):
        SF.surface_stats(a, b)
    with pytest.raises(ValueError):
        SF.surface_distances(a, b)


def test_instances_without_rows_and_without_bits_on_either_side():
    st, d = _case("hollow")
    a, b, _ = SI.get("hollow")
    assert st.count[:, 0].reshape(4, 3)[:, 0].tolist() == [0, 0, st.count[6, 0], 0] and st.count[6, 0] > 0
    none = (st.count == 0).any(1)
    assert none.sum() == 11 and (st.max_d2[none] == -1).all() and (st.argmax[none] == -1).all() and not st.within[none].any()
    assert (d.slot(6, 0) < SF.NONE).all() and (d.slot(7, 0) == SF.NONE).all() and len(d.slot(7, 0)) == st.count[6, 0]
    _surface(a)
    _surface(b)
    # sets without a single row, and without a single bit
    rowless, bitless = a.take([0, 3]), a.take([1])
    for x, y in ((rowless, rowless), (rowless, b), (b, rowless), (bitless, bitless), (bitless, b)):
        _stats(x, y, None, SF.surface_stats_numpy(x, y, None, SI.TAU2))
        _dist(x, y, None, SF.surface_distances_numpy(x, y))
    assert _surface(rowless).bits.size == 0


def test_pairs_repeated_and_reversed_and_no_pair_no_instance():
    a, b, _ = SI.get("empty_rows")
    pairs = np.array([[3, 0], [0, 0], [3, 0], [2, 0], [1, 0], [0, 0]], np.int32)
    st = _stats(a, b, pairs, SF.surface_stats_numpy(a, b, pairs, SI.TAU2))
    d = _dist(a, b, pairs, SF.surface_distances_numpy(a, b, pairs))
    assert _bytes(t[0] for t in st[:5]) == _bytes(t[2] for t in st[:5]) and np.array_equal(d.slot(1, 1), d.slot(5, 1))
    full = SI.stats_ref("empty_rows")
    assert np.array_equal(st.sum_d2[[1, 4, 3, 0]], full.sum_d2)
    none, nobody = np.zeros((0, 2), np.int32), SI.empty_set()
    for x, y, p in ((a, b, none), (nobody, b, None), (a, nobody, None), (nobody, nobody, None)):
        st = _stats(x, y, p, SF.surface_stats_numpy(x, y, p, SI.TAU2))
        d = _dist(x, y, p, SF.surface_distances_numpy(x, y, p))
        assert st.count.shape == (0, 2) and st.argmax.shape == (0, 2, 2) and st.within.shape == (0, 2, len(SI.TAU2))
        assert d.ptr.tolist() == [0] and d.d2.shape == (0,)
    assert len(_surface(nobody)) == 0
    no_tau = _stats(a, b, None, SF.surface_stats_numpy(a, b), tau2=())
    assert no_tau.within.shape == (4, 2, 0)


def test_the_methods_and_the_wrappers_agree():
    a, b, _ = SI.get("empty_rows")
    assert SI.same_fields(a.surface_stats(b, None, SI.TAU2), SI.stats_ref("empty_rows"))
    assert SI.same_fields(MT.mask_surface_stats(a, b, None, SI.TAU2), SI.stats_ref("empty_rows"))
    assert SI.same_fields(a.surface_distances(b), SI.dist_ref("empty_rows"))
    assert SI.same_fields(MT.mask_surface_distances(a, b), SI.dist_ref("empty_rows"))
    assert SI.same_set(a.surface(), SF.surface_numpy(a)) and SI.same_set(MT.mask_surface(b), SF.surface_numpy(b))


# ---- against the existing kernels ----

@pytest.mark.parametrize("name", ["word_edges", "empty_rows", "many130", "hollow"])
def test_the_surface_is_the_mask_minus_its_erosion_by_the_cross(name):
    pm = SI.get(name)[0]
    got, want = pm.surface().tighten(), pm - pm.erode(r2=1)
    assert SI.same_set(got, want) and got.areas.sum() > 0


@pytest.mark.parametrize("name", ["word_edges", "empty_rows", "ring", "large"])
def test_within_is_the_area_of_the_surface_and_the_dilated_other_surface(name):
    a, b, pairs = SI.get(name)
    pairs = SF._check_pairs("test", a, b, pairs)
    st = SF.surface_stats(a, b, pairs, SI.TAU2[:5])
    sa, sb = a.surface().take(pairs[:, 0]), b.surface().take(pairs[:, 1])
    for t, r2 in enumerate(SI.TAU2[:5]):
        assert np.array_equal(st.within[:, 0, t], (sa & sb.dilate(r2=r2)).areas)
        assert np.array_equal(st.within[:, 1, t], (sb & sa.dilate(r2=r2)).areas)
    assert st.within[:, :, 4].sum() > st.within[:, :, 0].sum()


# ---- the refusals ----

def _raw(entry, a, b=None, pairs=None, tau=(), cap=None, **kw):
    """One entry as it is, every output between canaries -> (status, the outputs).  kw: n, m, P, T replace the counts; null names
    the outputs (or "pairs", "tau2") handed over as NULL."""
    lib = _lib.load()
    null = kw.get("null", ())
    pairs = np.ascontiguousarray(pairs if pairs is not None else np.zeros((0, 2)), np.int32)
    tau = np.ascontiguousarray(tau, np.int32)
    P, T = kw.get("P", len(pairs)), kw.get("T", len(tau))
    room, t_room = max(len(pairs), 1), max(len(tau), 1)
    sa = list(_set_args(a, areas=False))
    sa[4] = kw.get("n", sa[4])
    if entry == "surface":
        n = len(a)
        outs = {"bounds": np.full((n + 1, 4), CANARY32, np.int32), "offsets": np.full(n + 1, CANARY64, np.int64),
                "areas": np.full(n + 1, CANARY64, np.int64), "bits": np.full(a.bits.size + 1, CANARY64, np.uint64),
                "need": np.full(1, CANARY64, np.uint64)}
        p = {k: (None if k in null else _lib.ptr(v)) for k, v in outs.items()}
        rc = lib.mnc_mask_surface(*(sa + [p["bounds"], p["offsets"], p["areas"], p["bits"], a.bits.nbytes if cap is None else cap,
                                          p["need"], 0]))
        return rc, outs
    sb = list(_set_args(b, areas=False))
    sb[4] = kw.get("m", sb[4])
    head = sa + sb + [None if "pairs" in null else _lib.ptr(pairs), P]
    if entry == "stats":
        outs = {"count": np.full((room, 2), CANARY64, np.int64), "max_d2": np.full((room, 2), CANARY64, np.int64),
                "argmax": np.full((room, 2, 2), CANARY32, np.int32), "sum_d2": np.full((room, 2), CANARY64, np.int64),
                "within": np.full((room, 2, t_room), CANARY64, np.int64)}
        p = {k: (None if k in null else _lib.ptr(v)) for k, v in outs.items()}
        rc = lib.mnc_mask_surface_stats(*(head + [None if "tau2" in null else _lib.ptr(tau), T, p["count"], p["max_d2"], p["argmax"],
                                                  p["sum_d2"], p["within"], 0]))
        return rc, outs
    outs = {"ptr": np.full(2 * room + 1, CANARY64, np.int64), "d2": np.full(4096 if cap is None else max(cap, 1), CANARY32, np.uint32),
            "total": np.full(1, CANARY64, np.uint64)}
    p = {k: (None if k in null else _lib.ptr(v)) for k, v in outs.items()}
    rc = lib.mnc_mask_surface_dist(*(head + [p["ptr"], p["d2"], outs["d2"].size if cap is None else cap, p["total"], 0]))
    return rc, outs


def _intact(outs, but=()):
    return all((a == (CANARY32 if a.dtype.itemsize == 4 else CANARY64)).all() for k, a in outs.items() if k not in but)


def test_bad_arguments_are_refused_before_anything_is_launched_with_nothing_written():
    a, b = SI.sectors_sets()
    ok = [[0, 0], [8, 0]]
    for entry in ("stats", "dist"):
        rc, outs = _raw(entry, a, b, ok, [4])
        assert rc == 0 and not _intact(outs)
        bad = [dict(pairs=[[0, 1]]), dict(pairs=[[9, 0]]), dict(pairs=[[-1, 0]]), dict(pairs=ok, P=-1), dict(pairs=ok, P=65537),
               dict(pairs=ok, null=("pairs",)), dict(pairs=ok, n=-1), dict(pairs=ok, n=2049), dict(pairs=ok, m=-1), dict(pairs=ok, m=2049)]
        if entry == "stats":
            bad += [dict(pairs=ok, tau=[-1]), dict(pairs=ok, tau=[1], T=9), dict(pairs=ok, tau=[1], T=-1), dict(pairs=ok, tau=[1], null=("tau2",))]
            bad += [dict(pairs=ok, tau=[1], null=(k,)) for k in ("count", "max_d2", "argmax", "sum_d2", "within")]
        else:
            bad += [dict(pairs=ok, null=("ptr",)), dict(pairs=ok, null=("total",))]
        for kw in bad:
            rc, outs = _raw(entry, a, b, **kw)
            assert rc == INVALID and _intact(outs), (entry, kw)
    one = np.ones((1, 1), bool)
    far = PackedMasks([[2 ** 24, 0, 2 ** 24 + 3, 4]], [0], [0], None, None, np.zeros(8, np.uint64))
    big = PackedMasks([[0, 0, 8192, 8192]], [0], [0], None, None, np.zeros(8, np.uint64))        # more than 2^26 pixels in a bound
    odd = PackedMasks(a.bounds, a.offsets + 4, a.areas, None, None, np.zeros(16, np.uint64))
    short = PackedMasks(a.bounds, a.offsets, a.areas, None, None, a.bits[:-1])
    wide = (SI._pack([(-16384, 0, one)]), SI._pack([(16383, 0, one)]))                           # a span of 32768 columns
    tall = (SI._pack([(0, -16384, one)]), SI._pack([(0, 16383, one)]))
    neg = PackedMasks(a.bounds, a.offsets - 8, a.areas, None, None, np.zeros(16, np.uint64))     # the first offset is -8
    rows2049 = SI._pack([(k % 100, k // 100, one) for k in range(2049)])                         # 2049 instances that have rows
    for x, y in ((far, b), (b, far), (big, b), (odd, b), (b, odd), (neg, b), (b, neg), (rows2049, b), (b, rows2049), (short, b), wide,
                 tall):
        for entry in ("stats", "dist"):
            rc, outs = _raw(entry, x, y, [[0, 0]], [4])
            assert rc == INVALID and _intact(outs), entry
    for pm in (far, big, odd, neg, rows2049, short, SI._pack([(-16384, 0, one), (16383, 5, one)])):
        rc, outs = _raw("surface", pm)
        assert rc == INVALID and _intact(outs)
    for kw in (dict(n=-1), dict(n=2049), dict(null=("need",)), dict(null=("bounds",)), dict(null=("offsets",)), dict(null=("areas",))):
        rc, outs = _raw("surface", a, **kw)
        assert rc == INVALID and _intact(outs), kw
    rc, outs = _raw("stats", *wide, pairs=[[0, 0]])
    assert rc == INVALID and b"span" in _lib.load().mnc_last_error()
    # the Python surface: ValueError
    for x, y in ((far, b), (big, b), wide, tall):
        with pytest.raises(ValueError):
            x.surface_stats(y, [[0, 0]])
        with pytest.raises(ValueError):
            x.surface_distances(y, [[0, 0]])
    for pm in (far, big, odd, neg, rows2049, short):
        with pytest.raises(ValueError):
            pm.surface()
    with pytest.raises(ValueError):
        a.surface_stats(b, [[0, 1]])
    with pytest.raises(ValueError):
        a.surface_stats(b, None, [-1])


def test_more_than_2_to_the_27_pixels_of_rows_are_refused_before_anything_is_launched():
    """Three bounds of 8192 x 8191 pixels, each within the 2^26 of one bound, over one block of zero words: 1.5 x 2^27 pixels.  Two of
    them are within the limit: the sizes-only call, which launches nothing, accepts them."""
    a, b = SI.sectors_sets()
    words = np.zeros(8191 * 128, np.uint64)
    three = PackedMasks([[0, 0, 8191, 8190]] * 3, [0] * 3, [0] * 3, None, None, words)
    two = PackedMasks([[0, 0, 8191, 8190]] * 2, [0] * 2, [0] * 2, None, None, words)
    one = PackedMasks([[0, 0, 8191, 8190]], [0], [0], None, None, words)
    assert 2 * 8192 * 8191 <= SF.MAX_PIXELS < 3 * 8192 * 8191 and 8192 * 8191 <= 2 ** 26
    for entry, sets in (("surface", (three,)), ("stats", (three, b)), ("stats", (b, three)), ("dist", (three, b)), ("dist", (two, one))):           # (the last: the pixels of both sets together)
        rc, outs = _raw(entry, *sets, pairs=[[0, 0]])
        assert rc == INVALID and _intact(outs) and b"pixels of rows" in _lib.load().mnc_last_error(), entry
    rc, outs = _raw("surface", two, null=("bits", "areas"))
    assert rc == 0 and outs["need"][0] == 2 * words.nbytes
    for call in (three.surface, lambda: three.surface_stats(b, [[0, 0]]), lambda: b.surface_distances(three, [[0, 0]])):
        with pytest.raises(ValueError):
            call()


def test_more_than_2_to_the_28_raw_distances_are_refused_after_the_read_back_with_nothing_written():
    """One 129 x 65 random instance against itself in 65536 pairs: 131072 slots of about 4000 surface pixels.  Only the surface
    kernel runs; the counts come back; the host refuses before it writes ptr or the total.  The greatest number of pairs within
    the limit is accepted by the sizes-only call."""
    a = SI._pack([(0, 0, SI._random(np.random.default_rng(2206), 65, 129))])
    count = int(SF.surface_numpy(a).areas[0])
    pairs = np.zeros((65536, 2), np.int32)
    assert count > 2048 and 2 * len(pairs) * count > SF.MAX_ENTRIES
    for null in ((), ("d2",)):
        rc, outs = _raw("dist", a, a, pairs, null=null)
        assert rc == INVALID and _intact(outs) and b"distances" in _lib.load().mnc_last_error()
    with pytest.raises(ValueError):
        a.surface_distances(a, pairs)
    fit = SF.MAX_ENTRIES // (2 * count)
    rc, outs = _raw("dist", a, a, pairs[:fit], null=("d2",))
    assert rc == 0 and outs["total"][0] == 2 * fit * count and outs["ptr"][-1] == 2 * fit * count and outs["ptr"][1] == count
    rc, outs = _raw("dist", a, a, pairs[:fit + 1], null=("d2",))
    assert rc == INVALID and _intact(outs)


def test_the_sizes_come_without_room_and_too_small_a_room_is_refused():
    a, b, _ = SI.get("empty_rows")
    pairs = SF._check_pairs("test", a, b, None)
    want = SI.dist_ref("empty_rows")
    rc, outs = _raw("dist", a, b, pairs, null=("d2",))
    assert rc == 0 and np.array_equal(outs["ptr"], want.ptr) and outs["total"][0] == want.ptr[-1] and _intact(outs, ("ptr", "total"))
    total = int(want.ptr[-1])
    rc, outs = _raw("dist", a, b, pairs, cap=total - 1)
    assert rc == INVALID and np.array_equal(outs["ptr"], want.ptr) and outs["total"][0] == total and _intact(outs, ("ptr", "total"))
    rc, outs = _raw("dist", a, b, pairs, cap=total + 3)                # entries past the total are never written
    assert rc == 0 and np.array_equal(outs["d2"][:total], want.d2) and (outs["d2"][total:] == CANARY32).all()
    s = SF.surface_numpy(a)
    rc, outs = _raw("surface", a, null=("bits", "areas"))
    assert rc == 0 and outs["need"][0] == s.bits.nbytes and np.array_equal(outs["offsets"][:-1], s.offsets) and _intact(outs, ("need", "offsets", "bounds"))
    rc, outs = _raw("surface", a, cap=s.bits.nbytes - 8)
    assert rc == INVALID and outs["need"][0] == s.bits.nbytes and _intact(outs, ("need", "offsets", "bounds"))
    rc, outs = _raw("surface", a)
    assert rc == 0 and np.array_equal(outs["bits"][:-1], s.bits) and outs["bits"][-1] == CANARY64 and outs["areas"][-1] == CANARY64
    assert np.array_equal(outs["areas"][:-1], s.areas) and (outs["bounds"][-1] == CANARY32).all()


def test_the_timer_keeps_the_kernels_time():
    a, b, _ = SI.get("empty_rows")
    SF.timing(True)
    try:
        a.surface_stats(b, None, [4])
        first = SF.timing(True)
        a.surface_distances(b)
        second = SF.timing(True)
        a.surface()
        third = SF.timing(False)
    finally:
        SF.timing(False)
    assert first > 0.0 and second > 0.0 and third > 0.0


# ---- the tool ----

def test_eval_coco_surface_on_the_gpu_prints_the_cpu_lines(tmp_path):
    import io
    from contextlib import redirect_stdout

    import eval_coco
    import mask_boundary_inputs as BI
    gt_path, dt_path, _ = BI.coco_files(tmp_path)
    got = {}
    for key, flags in (("gpu", []), ("cpu", ["--cpu"])):
        out = io.StringIO()
        with redirect_stdout(out):
            ev = eval_coco.main(["--gt", gt_path, "--dt", dt_path, "--surface"] + flags)
        got[key] = (out.getvalue().splitlines(), ev.surface)
    assert got["gpu"] == got["cpu"] and len(got["gpu"][0]) == 16 and got["gpu"][1]["pairs"] > 10
