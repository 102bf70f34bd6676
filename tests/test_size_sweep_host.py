"""CPU: the size list of the sweep (tests/size_sweep_inputs.py) really has the properties tests/test_gpu_size_sweep.py relies on --
derived with the ORACLE's prep and the ceil-mode pooling chain, nothing of the product -- and the oracle's own ProposalLayer answer
for the two entries with fewer anchors than RPN_PRE_NMS_TOP_N, so that the row counts the device must produce there are the
oracle's, not an assumption."""
import numpy as np
import pytest

import size_sweep_inputs as S
from oracle import host as ohost


def _entries():
    return [(h, w) + S.net_input(h, w) for h, w, _ in S.SIZES]


def test_the_list_names_the_sizes_a_voc_run_feeds():
    sizes = [(h, w) for h, w, _ in S.SIZES]
    assert len(set(sizes)) == len(sizes) and len({s for _, _, s in S.SIZES}) == len(sizes)
    for common in ((375, 500), (500, 375), (333, 500), (500, 333), (500, 500)):
        assert common in sizes
    got = {(h, w): (H, W, round(sc, 4)) for h, w, H, W, sc in _entries()}
    # the reference rule: short side -> 600 unless the long side would pass 1000 (figures of the oracle's prep)
    assert got[(375, 500)] == (600, 800, 1.6) and got[(500, 375)] == (800, 600, 1.6)
    assert got[(333, 500)] == (600, 901, 1.8018) and got[(500, 333)] == (901, 600, 1.8018)
    assert got[(500, 500)] == (600, 600, 1.2) and got[(281, 500)] == (562, 1000, 2.0)
    assert got[(1200, 1600)] == (600, 800, 0.5) and got[(120, 100)] == (720, 600, 6.0)
    # panoramas capped at MAX_SIZE, landscape and portrait: the short side of the net input is below 600
    assert any(W == 1000 and H < 600 for _, _, H, W, _ in _entries())
    assert any(H == 1000 and W < 600 for _, _, H, W, _ in _entries())
    assert all(max(H, W) <= 1000 and (min(H, W) == 600 or max(H, W) == 1000) for _, _, H, W, _ in _entries())
    # a scale below 1 (prep scales down: an image larger than the net input), one above 2 (an image below 300 on its long side)
    assert any(sc < 1.0 and min(h, w) > 600 for h, w, _, _, sc in _entries())
    assert any(sc > 2.0 and max(h, w) < 300 for h, w, _, _, sc in _entries())
    # no entry is the size every other full-width test runs
    assert all((H, W) != (600, 1000) and sc != 1.0 for _, _, H, W, sc in _entries())


def test_the_list_varies_the_chain_of_map_sizes():
    chains = [S.chain(H, W) for _, _, H, W, _ in _entries()]
    # (1200x1600 lands on 375x500's net input: the same trunk shapes, counted once)
    assert len({c[4] for c in chains}) >= 8
    assert len({tuple(c) for c in chains}) >= 8
    for level in range(5):            # net input, after pool1 .. pool4: an odd height and an odd width somewhere in the list
        assert any(c[level][0] % 2 == 1 for c in chains), level
        assert any(c[level][1] % 2 == 1 for c in chains), level
    # the odd VOC size: odd at several levels of ONE chain
    assert sum(1 for hh, _ in S.chain(562, 1000) if hh % 2) >= 3
    assert [S.pool_out(n) for n in (75, 125, 600, 2, 3, 901)] == [38, 63, 300, 1, 2, 451]
    # the run order goes up AND down in the net input's area, so buffers both grow and shrink along it (and along its reverse)
    area = [H * W for _, _, H, W, _ in _entries()]
    steps = np.sign(np.diff(area))
    assert (steps > 0).sum() >= 3 and (steps < 0).sum() >= 3


def test_trunk_shapes_follow_the_prototxt():
    shapes = S.trunk_shapes(600, 1000)
    assert [s[0] for s in shapes] == list(S.TRUNK_LAYERS) and len(shapes) == 13
    assert shapes[0] == ("conv1_1", 600, 1000, 3, 64) and shapes[1] == ("conv1_2", 600, 1000, 64, 64)
    assert shapes[4] == ("conv3_1", 150, 250, 128, 256) and shapes[7] == ("conv4_1", 75, 125, 256, 512)
    assert shapes[12] == ("conv5_3", 38, 63, 512, 512)
    # the widths are those of the full-width weights the GPU tests run
    from mnc_amd import models, synth
    wts = synth.synthetic_weights(models.write_mnc_5stage_test_prototxt(), seed=0)
    for name, _, _, cin, cout in shapes:
        assert wts[name][0].shape == (cout, cin, 3, 3), name
    cases = S.sweep_conv_cases()
    assert len(cases) == len({c[1:] for c in cases})
    assert {c[1] for c in cases} == {"c3", "pool", "plain"}
    assert all((c[1] == "c3") == (c[0] == "conv1_1") and (c[1] == "pool") == (c[0] in S.POOL_AFTER) for c in cases)
    # every layer class of every distinct net input is there; none of them is a shape the 600x1000 trunk launches
    inputs = {(H, W) for _, _, H, W, _ in _entries()}
    # 13 layers, conv5_1 = conv5_2 = conv5_3: 7 classes in stages 3-5 for every input, 4 in stages 1-2 for all but the skipped ones
    assert set(S.OP_LEVEL_SKIP_STAGE12) < inputs
    assert len(cases) == 7 * len(inputs) + 4 * (len(inputs) - len(S.OP_LEVEL_SKIP_STAGE12))
    for kind in ("c3", "pool"):        # partial 4x4 tiles along both edges stay in the full-resolution layers
        assert any(c[1] == kind and c[5] == 64 and c[2] % 4 for c in cases) and any(c[1] == kind and c[5] == 64 and c[3] % 4 for c in cases)
    base = {s[1:] for s in shapes}
    assert not any(c[2:] in base for c in cases)


def test_the_cases_the_throughput_plan_runs_in_the_split_form():
    """conv4_2 (plain) and conv4_3 (pool) of eight net inputs: 361 to 576 tiles, always two row blocks under the batched launch's
    304-row cut, K = N = 512.  conv4_1 (256 channels in), every conv5 map and the two panoramas' conv4 maps (below 304
    tiles) stay fused."""
    cases = S.split_cases()
    maps = [(75, 100), (90, 75), (75, 113), (125, 71), (100, 75), (71, 125), (75, 75), (113, 75)]
    assert cases == [(layer, kind, H, W, 512, 512) for H, W in maps for layer, kind in (("conv4_2", "plain"), ("conv4_3", "pool"))]
    assert len(cases) == 16 and len(S.sweep_conv_cases()) == 94
    tiles = [-(-c[2] // 4) * -(-c[3] // 4) for c in cases]
    assert min(tiles) == 361 and max(tiles) == 576
    assert all(-(-t // 304) == -(-t // 320) == 2 for t in tiles)          # two blocks, the 304-row cut on
    rest = [c for c in S.sweep_conv_cases() if c not in cases]
    assert all(c[4] < 512 or -(-c[2] // 4) * -(-c[3] // 4) < 304 for c in rest)


def test_the_entries_with_fewer_anchors_than_pre_nms_top_n():
    sizes = [(a, b) for a, b, _ in S.SIZES]
    assert S.UNDER_6000 in sizes and S.FEW_ROIS in sizes
    assert S.net_input(*S.UNDER_6000) == (150, 1000, 2.0) and S.feature_map(*S.UNDER_6000) == (10, 63)
    assert S.anchors(*S.UNDER_6000) == 5670 < ohost.RPN_PRE_NMS_TOP_N == 6000
    assert S.net_input(*S.FEW_ROIS) == (60, 1000, 2.0) and S.feature_map(*S.FEW_ROIS) == (4, 63)
    assert S.anchors(*S.FEW_ROIS) == 2268
    assert all(S.anchors(a, b) > ohost.RPN_PRE_NMS_TOP_N for a, b in sizes if (a, b) not in (S.UNDER_6000, S.FEW_ROIS))


# What the oracle's ProposalLayer returned on its own RPN blobs for the two entries when this was written (full width,
# synthetic_weights(seed=0), the entry's own image; printed on every run): candidates after the min-size filter, rois after
# NMS(0.7)[:300].  A box that sits on the min-size or the IoU threshold can fall the other way under another CPU's summation order,
# so the test holds the counts to what the GPU test relies on -- 300 rows / clearly fewer than 300 -- and not to the last unit.
ORACLE_PROPOSALS = {S.UNDER_6000: (5591, 300), S.FEW_ROIS: (2223, 125)}


@pytest.mark.parametrize("size", [S.UNDER_6000, S.FEW_ROIS])
def test_oracle_proposals_where_the_top_k_cut_cannot_happen(size):
    """The oracle up to the ProposalLayer on the entry's image, full width.  Fewer candidates than RPN_PRE_NMS_TOP_N: the top-k is
    a full sort.  At 150x1000 the NMS still keeps more than 300 (the device must return 300 rows); on the 60x1000 strip it keeps
    125 -- the device has to run its heads on fewer rows than post_nms_topN there (tests/test_gpu_size_sweep.py holds the device's
    rois to proposal_forward on the device's own blobs, which differ from the oracle's in the last bits: the count recorded here is
    far enough from 300 for `fewer than 300` to be the oracle's statement, not an assumption)."""
    from mnc_amd import models, synth
    from oracle import net as onet
    h, w = size
    seed = [s for a, b, s in S.SIZES if (a, b) == size][0]
    wts = synth.synthetic_weights(models.write_mnc_5stage_test_prototxt(), seed=0)
    data, im_info, scale = ohost.prepare_mnc_args(S.image(h, w, seed))
    assert data.shape[2:] == S.net_input(h, w)[:2] and scale == 2.0
    c5 = onet.trunk(wts, data)
    fh, fw = S.feature_map(h, w)
    assert tuple(c5.shape[2:]) == (fh, fw)
    prob, bbox = onet.rpn(wts, c5)
    assert prob.shape == (1, 18, fh, fw) and bbox.shape == (1, 36, fh, fw)
    cand, scores = ohost.proposal_candidates(prob, bbox, im_info)
    assert len(cand) == len(scores) <= S.anchors(h, w) < ohost.RPN_PRE_NMS_TOP_N
    assert np.all(np.diff(scores.ravel()) <= 0)
    rois = ohost.proposal_forward(prob, bbox, im_info)
    print("oracle, %dx%d -> %dx%d: %d candidates of %d anchors, %d rois" % (h, w, data.shape[2], data.shape[3], len(cand),
                                                                          S.anchors(h, w), len(rois)))
    assert rois.shape[1] == 5 and 0.9 * S.anchors(h, w) < len(cand)
    if size == S.UNDER_6000:
        assert rois.shape[0] == ohost.RPN_POST_NMS_TOP_N == ORACLE_PROPOSALS[size][1]
    else:
        assert 0 < rois.shape[0] < ohost.RPN_POST_NMS_TOP_N // 2 and abs(rois.shape[0] - ORACLE_PROPOSALS[size][1]) <= 10
