#!/usr/bin/env python3
"""Time the way out of one image's instances and the way back: COCO run-length encoding of the voted instances' packed masks, in
host form (mnc_amd.rle.rle_counts_numpy: unpack every mask to a full canvas, flatten it column-major, diff it) against device form
(PackedMasks.rle_counts() of a device-resident InstanceView.masks() result, csrc/mask_rle.hip, with the copies of run_ptr and of
the runs to the host), and the decoding of those counts (masks_from_counts_numpy against mnc_mask_from_rle, host arrays in, host
arrays out), on a 600x1000 and a 375x500 synthetic image.  The instances are made as tools/mask_overlap_bench.py makes them.  The
encode kernels' own time comes from the context's event profile of the same call.  Medians over --iters device rounds and
--host-iters host rounds after one warm-up each; one JSON line.

    python tools/mask_rle_bench.py [--iters 20] [--host-iters 3] [--keep 100]
"""
import numpy as np

from _task_harness import emit, median_ms, parser, profiled_us, voted_instances


def main():
    args = parser().parse_args()
    from mnc_amd import rle
    sizes = []
    for H, W, t, host, thr in voted_instances("mask_rle_bench", args.keep, args.math):
        dev = t.net._inst.view().masks(H, W, score_thresh=thr)       # the device form's input: nothing copied yet
        n = len(dev)                                                 # (the instance table comes down here, the bits never)
        want, got = rle.rle_counts_numpy(host, H, W), dev.rle_counts(H, W)
        same = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))
        assert "bits" not in dev._host
        back_want = rle.masks_from_counts_numpy(want[0], want[1], H, W)
        back_got = rle.masks_from_counts(want[0], want[1], H, W)
        same_back = all(np.array_equal(getattr(back_want, f), getattr(back_got, f)) for f in ("bounds", "offsets", "areas", "bits"))
        enc_host = median_ms(lambda: rle.rle_counts_numpy(host, H, W), args.host_iters, t.net.sync)
        enc_dev = median_ms(lambda: dev.rle_counts(H, W), args.iters, t.net.sync)
        dec_host = median_ms(lambda: rle.masks_from_counts_numpy(want[0], want[1], H, W), args.host_iters, t.net.sync)
        dec_dev = median_ms(lambda: rle.masks_from_counts(want[0], want[1], H, W), args.iters, t.net.sync)
        str_host = median_ms(lambda: rle._to_rles(want[0], want[1], H, W), args.host_iters, t.net.sync)
        sizes.append({"image": "%dx%d" % (H, W), "instances": n, "score_thresh": thr, "runs": int(len(want[1])),
                      "bits_bytes": int(host.bits.nbytes), "encode_device_equals_host": same,
                      "decode_device_equals_host": bool(same_back),
                      "encode_host_ms_median": enc_host[0], "encode_host_ms_min": enc_host[1],
                      "encode_device_ms_median": enc_dev[0], "encode_device_ms_min": enc_dev[1],
                      # the context's event pair around the encoder's five launches
                      "encode_kernels_us_median": profiled_us(t.net, "mask_rle", lambda: dev.rle_counts(H, W), args.iters),
                      "decode_host_ms_median": dec_host[0], "decode_host_ms_min": dec_host[1],
                      "decode_device_ms_median": dec_dev[0], "decode_device_ms_min": dec_dev[1],
                      "counts_to_strings_ms_median": str_host[0]})
    emit({"workload": "COCO run-length encoding of mnc 5-stage vgg16's voted instances at image resolution, and back",
          "host": "rle_counts_numpy / masks_from_counts_numpy on a host PackedMasks",
          "device": "PackedMasks.rle_counts() of a device-resident result + copies of run_ptr and the runs; "
                    "mnc_mask_from_rle from host counts to host arrays",
          "device_rounds": max(args.iters, 1), "host_rounds": max(args.host_iters, 1), "sizes": sizes})


if __name__ == "__main__":
    main()
