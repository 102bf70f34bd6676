#!/usr/bin/env python3
"""Re-evaluate a finished `tools/test_net.py --task seg|cfm` run: the res_boxes.pkl / res_masks.pkl it left in its output
directory -> imdb.evaluate_segmentation, the SDS mAP^r at 0.5 and 0.7, without building a network.  By default the pixel
counting runs on the GPU (utils/voc_eval.py:voc_eval_sds_device, one device call for all classes and both thresholds);
`--cpu` runs the CPU loop (voc_eval_sds).  The APs are the same either way.

    python tools/eval_seg.py --imdb voc_2012_seg_val --output-dir output/default/voc_2012_seg_val/mnc_model [--cpu]

(`test_net.py` itself evaluates on the GPU with `--cfg` pointing at a file that sets `TEST: {USE_GPU_SDS_EVAL: True}`.)
"""
import argparse
import os
import pickle
import sys

import _init_paths  # noqa: F401
from db.imdb import get_imdb
from mnc_config import cfg, cfg_from_file


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Re-evaluate the result pickles of a seg / cfm test run (SDS mAP^r)')
    parser.add_argument('--imdb', dest='imdb_name', help='dataset the run was tested on', default='voc_2012_seg_val', type=str)
    parser.add_argument('--output-dir', dest='output_dir', required=True, help='directory holding res_boxes.pkl / res_masks.pkl')
    parser.add_argument('--cfg', dest='cfg_file', help='optional config file', default=None, type=str)
    parser.add_argument('--gpu', dest='gpu_id', help='GPU id to use', default=0, type=int)
    parser.add_argument('--cpu', dest='cpu', action='store_true', help='count the overlaps with the CPU loop (voc_eval_sds)')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.cfg_file is not None:
        cfg_from_file(args.cfg_file)
    cfg.GPU_ID = args.gpu_id
    with open(os.path.join(args.output_dir, 'res_boxes.pkl'), 'rb') as f:
        seg_box = pickle.load(f)
    with open(os.path.join(args.output_dir, 'res_masks.pkl'), 'rb') as f:
        seg_mask = pickle.load(f)
    imdb = get_imdb(args.imdb_name)
    return imdb.evaluate_segmentation(seg_box, seg_mask, args.output_dir, on_device=not args.cpu)


if __name__ == '__main__':
    main(sys.argv[1:])
