#!/usr/bin/env python3
"""Time COCO's matching of one image's detections to its ground truths (mnc_amd/coco_eval.py, csrc/mask_match.hip): the numpy
statement (match_numpy: unpack, slice and sum per pair, then evaluateImg's triple loop) on a host PackedMasks against
PackedMasks.match() of a device-resident InstanceView.masks() result, with its copies of the five tables to the host, and the
device time of the launches alone -- on a 600x1000 and a 375x500 synthetic image.  The detections are made as
tools/mask_overlap_bench.py makes them: the 5-stage VGG-16 graph with seeded synthetic weights, gpu_mask_voting, the --keep
best-scoring instances (synthetic weights give meaningless scores).  The ground truths are synthetic too: --gts of those
instances, evenly spaced, every tenth of them a crowd; default thresholds and area ranges (T = 10, A = 4), max_det = 100.
Medians over --iters device rounds and --host-iters host rounds after one warm-up each; one JSON line.

    python tools/mask_match_bench.py [--iters 20] [--host-iters 3] [--keep 100] [--gts 20]
"""
import numpy as np

from _task_harness import emit, median_ms, parser, profiled_us, voted_instances


def main():
    ap = parser()
    ap.add_argument("--gts", type=int, default=20)
    args = ap.parse_args()
    from mnc_amd.coco_eval import Match, match_numpy
    sizes = []
    for H, W, t, host, thr in voted_instances("mask_match_bench", args.keep, args.math):
        dev = t.net._inst.view().masks(H, W, score_thresh=thr)       # the device form's input: nothing copied yet
        n = len(dev)                                                 # (the instance table comes down here, the bits never)
        gt = host.take(np.linspace(0, n - 1, min(args.gts, n)).astype(int))
        crowd = (np.arange(len(gt)) % 10 == 9).astype(np.uint8)
        want, got = match_numpy(host, gt, crowd), dev.match(gt, crowd)
        same = all(np.array_equal(a, b) for a, b in zip(want[:5], got[:5]))
        assert "bits" not in dev._host
        m_host = median_ms(lambda: match_numpy(host, gt, crowd), args.host_iters, t.net.sync)
        m_dev = median_ms(lambda: dev.match(gt, crowd), args.iters, t.net.sync)
        sizes.append({"image": "%dx%d" % (H, W), "detections": n, "ground_truths": len(gt), "classes": int(len(np.unique(host.classes))),
                      "score_thresh": thr, "matches_at_iou50": int((want.dt_match[0, 0] >= 0).sum()),
                      "bits_bytes": int(host.bits.nbytes), "device_equals_host": bool(same),
                      "host_ms_median": m_host[0], "host_ms_min": m_host[1],
                      "device_ms_median": m_dev[0], "device_ms_min": m_dev[1],
                      # the context's event pair around the uploads, the fills and the four kernels
                      "kernels_us_median": profiled_us(t.net, "mask_match", lambda: dev.match(gt, crowd), args.iters)})
    emit({"workload": "COCO matching (T = 10, A = 4, max_det = 100) of mnc 5-stage vgg16's voted instances against "
                      "synthetic ground truths at image resolution",
          "host": "match_numpy on a host PackedMasks", "tables": list(Match._fields[:5]),
          "device": "PackedMasks.match() of a device-resident result + copies of the five tables",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes})


if __name__ == "__main__":
    main()
