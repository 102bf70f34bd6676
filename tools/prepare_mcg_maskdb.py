#!/usr/bin/env python3
"""Build the MCG proposal maskdb `tools/test_net.py --task cfm` reads, from the published MCG candidates (the validation branch
of the reference's tools/prepare_mcg_maskdb.py, same command line): per image of the list, <input>/<name>.mat (`superpixels`,
`labels`) -> <output>/<name>.mat ({'masks': bool [n, S, S], 'boxes': float64 [n, 4]}).  Files that exist are skipped.

    python tools/prepare_mcg_maskdb.py --input data/MCG-raw/ --output data/cache/voc_2012_val_mcg_maskdb/ --db val
                                       [--list data/VOCdevkitSDS/val.txt] [-mask_sz 21] [--top_k -1] [--para_job 1] [--cpu]

The boxes and masks are computed on the GPU (db/mcg_maskdb.py:mcg_maskdb_device, one call per image); `--cpu` runs the numpy
form of the reference's loop instead -- the files are the same.  Reading the MCG file and writing the result take far longer than
the device call, so `--para_job N` (at most 16 fresh processes, each with the GPU open) only spreads the file work.
`--db train` (GT overlaps, mask targets, flips) is not provided: training is out of this project's scope."""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

import _init_paths  # noqa: F401
from db.mcg_maskdb import mcg_maskdb_device, mcg_maskdb_numpy, read_mcg_raw, write_maskdb
from mnc_config import cfg

MAX_JOBS = 16
TRAIN_MESSAGE = ("prepare_mcg_maskdb: --db train is not provided -- preparing training data (GT overlaps, mask targets, flipped "
                 "copies) is out of scope; use --db val")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Prepare MCG roidb')
    parser.add_argument('--input', dest='input_dir', help='folder contain input mcg proposals', default='data/MCG-raw/', type=str)
    parser.add_argument('--output', dest='output_dir', help='folder contain output roidb', required=True, type=str)
    parser.add_argument('-mask_sz', dest='mask_size', help='compressed mask resolution', default=21, type=int)
    parser.add_argument('--top_k', dest='top_k', help='number of generated proposal', default=-1, type=int)
    parser.add_argument('--db', dest='db_name', help='train or validation', default='train', type=str)
    parser.add_argument('--para_job', dest='para_job', help='launch several process', default=1, type=int)
    parser.add_argument('--list', dest='list_name', help='image list (default: data/VOCdevkitSDS/val.txt)', default=None, type=str)
    parser.add_argument('--cpu', dest='cpu', action='store_true', help='the numpy form of the loop instead of the GPU')
    parser.add_argument('--gpu', dest='gpu_id', help='GPU id to use', default=0, type=int)
    return parser.parse_args(argv)


def process_roidb(file_list, file_start, file_end, input_dir, output_dir, mask_size, top_k, cpu, gpu_id):
    """Images [file_start, file_end) of the list; -> files written."""
    cfg.GPU_ID = gpu_id
    written = 0
    for cnt in range(file_start, file_end):
        f = file_list[cnt]
        output_cache = os.path.join(output_dir, f.split('.')[0] + '.mat')
        timer_tic = time.time()
        if os.path.exists(output_cache):
            continue
        full_file = os.path.join(input_dir, f if f.endswith('.mat') else f + '.mat')
        superpixels, label_ptr, label_ids = read_mcg_raw(full_file)
        build = mcg_maskdb_numpy if cpu else mcg_maskdb_device
        write_maskdb(output_cache, build(superpixels, label_ptr, label_ids, mask_size=mask_size, top_k=top_k))
        written += 1
        print('%d/%d use time %f' % (cnt, len(file_list), time.time() - timer_tic))
    return written


def main(argv=None):
    args = parse_args(argv)
    if args.db_name == 'train':
        sys.exit(TRAIN_MESSAGE)
    if args.db_name != 'val':
        sys.exit("prepare_mcg_maskdb: --db must be 'val' (got %r)" % args.db_name)
    assert os.path.exists(args.input_dir), 'Path does not exist: {}'.format(args.input_dir)
    if not os.path.isdir(args.output_dir):
        os.makedirs(args.output_dir)
    with open(args.list_name or 'data/VOCdevkitSDS/val.txt') as f:
        file_list = f.read().splitlines()
    work = (args.input_dir, args.output_dir, args.mask_size, args.top_k, args.cpu, args.gpu_id)
    num_process = max(1, min(args.para_job, MAX_JOBS, len(file_list)))
    if num_process == 1:
        process_roidb(file_list, 0, len(file_list), *work)
        return 0
    # fresh interpreters (spawn), never a fork: a child of a process that has opened the GPU must not inherit its state
    ctx = multiprocessing.get_context('spawn')
    file_offset = int(np.ceil(len(file_list) / float(num_process)))
    processes = []
    for file_start in range(0, len(file_list), file_offset):
        p = ctx.Process(target=process_roidb, args=(file_list, file_start, min(file_start + file_offset, len(file_list))) + work)
        p.start()
        processes.append(p)
    for p in processes:
        p.join()
    failed = [p.exitcode for p in processes if p.exitcode != 0]
    if failed:
        sys.exit('prepare_mcg_maskdb: %d of %d worker processes failed (exit codes %s)' % (len(failed), len(processes), failed))
    return 0


if __name__ == '__main__':
    main(sys.argv[1:])
