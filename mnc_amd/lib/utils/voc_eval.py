"""Instance-segmentation evaluation, mAP^r of SDS (reference: lib/utils/voc_eval.py:19-52 voc_ap, :195-283 voc_eval_sds,
:307-352 parse_inst, :355-393 check_voc_sds_cache; lib/transform/mask_transform.py:16-46 mask_overlap).  Python-3 port of
the caller on the output side of the hot path: pickles are binary, dict iteration is .items(),
cv2.resize is utils.blob.resize_to."""
import os
import pickle

import numpy as np

from mnc_config import cfg
from transform.mask_transform import mask_overlap
from utils.blob import resize_to


def voc_ap(rec, prec, use_07_metric=False):
    """AP from recall/precision: the VOC07 11-point interpolation, or the area under the precision envelope."""
    if use_07_metric:
        ap = 0.
        for t in np.arange(0., 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap += p / 11.
        return ap
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def parse_rec(filename):
    """Objects of a PASCAL VOC annotation file: name, pose, truncated, difficult, bbox [xmin, ymin, xmax, ymax]."""
    import xml.etree.ElementTree as ET
    objects = []
    for obj in ET.parse(filename).findall('object'):
        bbox = obj.find('bndbox')
        objects.append({'name': obj.find('name').text, 'pose': obj.find('pose').text,
                        'truncated': int(obj.find('truncated').text), 'difficult': int(obj.find('difficult').text),
                        'bbox': [int(bbox.find('xmin').text), int(bbox.find('ymin').text), int(bbox.find('xmax').text),
                                 int(bbox.find('ymax').text)]})
    return objects


def voc_eval(detpath, annopath, imagesetfile, classname, cachedir, ovthresh=0.5, use_07_metric=False):
    """PASCAL VOC detection AP of one class (reference: lib/utils/voc_eval.py:55-192): detpath.format(classname) is the
    results file (`image score x1 y1 x2 y2` per line), annopath.format(image) the XML annotation.  Returns rec, prec, ap."""
    if not os.path.isdir(cachedir):
        os.mkdir(cachedir)
    cachefile = os.path.join(cachedir, 'annots.pkl')
    with open(imagesetfile, 'r') as f:
        imagenames = [x.strip() for x in f.readlines()]
    if not os.path.isfile(cachefile):
        recs = {}
        for i, imagename in enumerate(imagenames):
            recs[imagename] = parse_rec(annopath.format(imagename))
            if i % 100 == 0:
                print('Reading annotation for {:d}/{:d}'.format(i + 1, len(imagenames)))
        print('Saving cached annotations to {:s}'.format(cachefile))
        with open(cachefile, 'wb') as f:
            pickle.dump(recs, f)
    else:
        with open(cachefile, 'rb') as f:
            recs = pickle.load(f)

    class_recs = {}
    npos = 0
    for imagename in imagenames:
        R = [obj for obj in recs[imagename] if obj['name'] == classname]
        bbox = np.array([x['bbox'] for x in R])
        difficult = np.array([x['difficult'] for x in R]).astype(bool)
        npos = npos + sum(~difficult)
        class_recs[imagename] = {'bbox': bbox, 'difficult': difficult, 'det': [False] * len(R)}

    with open(detpath.format(classname), 'r') as f:
        splitlines = [x.strip().split(' ') for x in f.readlines()]
    image_ids = [x[0] for x in splitlines]
    confidence = np.array([float(x[1]) for x in splitlines])
    BB = np.array([[float(z) for z in x[2:]] for x in splitlines])

    sorted_ind = np.argsort(-confidence)
    BB = BB[sorted_ind, :] if len(sorted_ind) else BB
    image_ids = [image_ids[x] for x in sorted_ind]

    nd = len(image_ids)
    tp = np.zeros(nd)
    fp = np.zeros(nd)
    for d in range(nd):
        R = class_recs[image_ids[d]]
        bb = BB[d, :].astype(float)
        ovmax = -np.inf
        BBGT = R['bbox'].astype(float)
        if BBGT.size > 0:
            ixmin = np.maximum(BBGT[:, 0], bb[0])
            iymin = np.maximum(BBGT[:, 1], bb[1])
            ixmax = np.minimum(BBGT[:, 2], bb[2])
            iymax = np.minimum(BBGT[:, 3], bb[3])
            iw = np.maximum(ixmax - ixmin + 1., 0.)
            ih = np.maximum(iymax - iymin + 1., 0.)
            inters = iw * ih
            uni = ((bb[2] - bb[0] + 1.) * (bb[3] - bb[1] + 1.) +
                   (BBGT[:, 2] - BBGT[:, 0] + 1.) * (BBGT[:, 3] - BBGT[:, 1] + 1.) - inters)
            overlaps = inters / uni
            ovmax = np.max(overlaps)
            jmax = np.argmax(overlaps)
        if ovmax > ovthresh:
            if not R['difficult'][jmax]:
                if not R['det'][jmax]:
                    tp[d] = 1.
                    R['det'][jmax] = 1
                else:
                    fp[d] = 1.
        else:
            fp[d] = 1.

    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    rec = tp / float(npos)
    prec = tp / (tp + fp)
    return rec, prec, voc_ap(rec, prec, use_07_metric)


def parse_inst(image_name, devkit_path):
    """Ground-truth instances of one SBD image: inst/<name>.mat (instance ids) + cls/<name>.mat (class ids) ->
    [{'mask': bool [h,w] inside its bounds, 'mask_cls': class id, 'mask_bound': [x1,y1,x2,y2]}]."""
    import scipy.io as sio
    inst = sio.loadmat(os.path.join(devkit_path, 'inst', image_name + '.mat'))['GTinst']['Segmentation'][0][0]
    cls = sio.loadmat(os.path.join(devkit_path, 'cls', image_name + '.mat'))['GTcls']['Segmentation'][0][0]
    record = []
    for inst_id in np.unique(inst):
        if inst_id == 0:                # background
            continue
        r, c = np.where(inst == inst_id)
        bound = np.array([np.min(c), np.min(r), np.max(c), np.max(r)], dtype=np.float64)
        x1, y1, x2, y2 = (int(v) for v in bound)
        mask = inst[y1:y2 + 1, x1:x2 + 1] == inst_id
        classes = np.unique(cls[y1:y2 + 1, x1:x2 + 1][mask])
        assert classes.shape[0] == 1
        record.append({'mask': mask, 'mask_cls': classes[0], 'mask_bound': bound})
    return record


def parse_inst_maps(inst, cls, on_device=False):
    """The records of parse_inst from the two arrays themselves (GTinst's and GTcls's Segmentation): the same keys, dtypes, bounds
    as float64 and order, made through mnc_amd.labels -- from_labels_numpy, or with on_device the GPU (mnc_label_table +
    mnc_label_masks) -- in place of one np.where per instance.  An instance of mixed class raises ValueError where parse_inst
    asserts."""
    from mnc_amd import labels
    inst, cls = np.asarray(inst), np.asarray(cls)
    pm, _ = (labels.from_labels if on_device else labels.from_labels_numpy)(inst, cls, 0)
    return [{'mask': pm.dense(k), 'mask_cls': cls.dtype.type(pm.classes[k]), 'mask_bound': pm.bounds[k].astype(np.float64)}
            for k in range(len(pm))]


def check_voc_sds_cache(cache_dir, devkit_path, image_names, class_names):
    """Builds <cache_dir>/<class>_mask_gt.pkl ({image: [instances]}) once."""
    if not os.path.isdir(cache_dir):
        os.mkdir(cache_dir)
    if all(os.path.isfile(os.path.join(cache_dir, n + '_mask_gt.pkl')) for n in class_names if n != '__background__'):
        return
    record_list = [{} for _ in range(len(class_names))]
    for i, image_name in enumerate(image_names):
        for mask_dic in parse_inst(image_name, devkit_path):
            mask_dic['already_detect'] = False
            record_list[int(mask_dic['mask_cls'])].setdefault(image_name, []).append(mask_dic)
        if i % 100 == 0:
            print('Reading annotation for {:d}/{:d}'.format(i + 1, len(image_names)))
    print('Saving cached annotations...')
    for cls_ind, name in enumerate(class_names):
        if name == '__background__':
            continue
        with open(os.path.join(cache_dir, name + '_mask_gt.pkl'), 'wb') as f:
            pickle.dump(record_list[cls_ind], f)


def voc_eval_sds(det_file, seg_file, devkit_path, image_list, cls_name, cache_dir, class_names, ov_thresh=0.5):
    """AP^r of one class: predictions ranked by score, a prediction is a true positive when its mask (21x21 resized to its
    box, binarised at cfg.BINARIZE_THRESH) overlaps a not-yet-matched ground-truth instance of the class by >= ov_thresh."""
    with open(image_list, 'r') as f:
        image_names = [x.strip() for x in f.readlines()]
    check_voc_sds_cache(cache_dir, devkit_path, image_names, class_names)
    with open(cache_dir + '/' + cls_name + '_mask_gt.pkl', 'rb') as f:
        gt_pkl = pickle.load(f)
    with open(det_file, 'rb') as f:
        boxes_pkl = pickle.load(f)
    with open(seg_file, 'rb') as f:
        masks_pkl = pickle.load(f)

    box_num = sum(len(boxes_pkl[i]) for i in range(len(image_names)))
    new_boxes = np.zeros((box_num, 5))
    new_masks = np.zeros((box_num, cfg.MASK_SIZE, cfg.MASK_SIZE))
    new_image = []
    cnt = 0
    for image_ind, name in enumerate(image_names):
        boxes, masks = boxes_pkl[image_ind], masks_pkl[image_ind]
        for box_ind in range(len(boxes)):
            new_boxes[cnt] = boxes[box_ind]
            new_masks[cnt] = masks[box_ind]
            new_image.append(name)
            cnt += 1

    keep_inds = np.argsort(-new_boxes[:, -1])
    new_boxes = new_boxes[keep_inds, :]
    new_masks = new_masks[keep_inds, :, :]
    num_pred = new_boxes.shape[0]

    fp = np.zeros((num_pred, 1))
    tp = np.zeros((num_pred, 1))
    for i in range(num_pred):
        pred_box = np.round(new_boxes[i, :4]).astype(int)
        pred_mask = resize_to(new_masks[i].astype(np.float32), pred_box[2] - pred_box[0] + 1, pred_box[3] - pred_box[1] + 1)
        pred_mask = pred_mask >= cfg.BINARIZE_THRESH
        image_index = new_image[keep_inds[i]]
        if image_index not in gt_pkl:
            fp[i] = 1
            continue
        gt_dict_list = gt_pkl[image_index]
        cur_overlap, cur_overlap_ind = -1000, -1
        for ind2, gt_dict in enumerate(gt_dict_list):
            ov = mask_overlap(np.round(gt_dict['mask_bound']).astype(int), pred_box, gt_dict['mask'], pred_mask)
            if ov > cur_overlap:
                cur_overlap, cur_overlap_ind = ov, ind2
        if cur_overlap >= ov_thresh and not gt_dict_list[cur_overlap_ind]['already_detect']:
            tp[i] = 1
            gt_dict_list[cur_overlap_ind]['already_detect'] = 1
        else:
            fp[i] = 1

    num_pos = sum(len(val) for val in gt_pkl.values())
    fp = np.cumsum(fp)
    tp = np.cumsum(tp)
    rec = tp / float(num_pos)
    prec = tp / np.maximum(fp + tp, np.finfo(np.float64).eps)
    return voc_ap(rec, prec, True)


# ---- the same evaluation with the pixel counting on the GPU (csrc/sds_eval.hip, mnc_sds_best_overlap) ----------------------
def sds_best_overlap(boxes, masks, gt_begin, gt_end, gt_bounds, gt_offsets, gt_bits, gt_areas, binarize_thresh, device_id=0):
    """mnc_sds_best_overlap: per prediction the arg-max GT of voc_eval_sds's overlap loop (-1: no GT of its class in its image)
    and that GT's pixel intersection / union.  boxes [P,4] float64, masks [P, S*S] uint8; GT i of the packed arrays is prediction
    p's for gt_begin[p] <= i < gt_end[p].  -> best_gt int32 [P], best_inter int64 [P], best_union int64 [P]."""
    from mnc_amd import _lib
    boxes = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 4)
    P = boxes.shape[0]
    masks = np.ascontiguousarray(masks, dtype=np.uint8).reshape(P, -1)
    S = int(round(np.sqrt(masks.shape[1]))) if P else cfg.MASK_SIZE
    if S * S != masks.shape[1]:
        raise ValueError('masks of %d values are not square' % masks.shape[1])
    gt_begin = np.ascontiguousarray(gt_begin, dtype=np.int32)
    gt_end = np.ascontiguousarray(gt_end, dtype=np.int32)
    if gt_begin.shape != (P,) or gt_end.shape != (P,):
        raise ValueError('gt_begin / gt_end must have one entry per prediction')
    gt_bounds = np.ascontiguousarray(gt_bounds, dtype=np.int32).reshape(-1, 4)
    G = gt_bounds.shape[0]
    gt_offsets = np.ascontiguousarray(gt_offsets, dtype=np.int64)
    gt_areas = np.ascontiguousarray(gt_areas, dtype=np.int64)
    gt_bits = np.ascontiguousarray(gt_bits, dtype=np.uint8)
    if gt_offsets.shape != (G,) or gt_areas.shape != (G,):
        raise ValueError('gt_offsets / gt_areas must have one entry per GT')
    best_gt = np.empty(P, np.int32)
    best_inter = np.empty(P, np.int64)
    best_union = np.empty(P, np.int64)
    _lib.call('mnc_sds_best_overlap', _lib.ptr(boxes), _lib.ptr(masks), P, S, _lib.ptr(gt_begin), _lib.ptr(gt_end), G,
              _lib.ptr(gt_bounds), _lib.ptr(gt_offsets), _lib.ptr(gt_bits), gt_bits.size, _lib.ptr(gt_areas),
              float(binarize_thresh), _lib.ptr(best_gt), _lib.ptr(best_inter), _lib.ptr(best_union), int(device_id))
    return best_gt, best_inter, best_union


def pack_sds_gt(gt_dicts):
    """Cached GT instances (check_voc_sds_cache's dicts, in order) -> the entry's GT arrays: bounds int32 [G,4] (the rounded
    mask_bound), byte offsets int64 [G], the bit rows of every mask (np.packbits(axis=1, bitorder='little')), areas int64 [G],
    and the instances' already_detect flags (bool [G])."""
    G = len(gt_dicts)
    bounds = np.zeros((G, 4), np.int32)
    offsets = np.zeros(G, np.int64)
    areas = np.zeros(G, np.int64)
    pre = np.zeros(G, bool)
    rows, nbytes = [], 0
    for i, gt in enumerate(gt_dicts):
        b = np.round(gt['mask_bound']).astype(int)
        m = np.asarray(gt['mask'], dtype=bool)
        if m.shape != (b[3] - b[1] + 1, b[2] - b[0] + 1):
            raise ValueError('GT mask of shape %s does not fill its bound %s' % (m.shape, b))
        bounds[i] = b
        offsets[i] = nbytes
        areas[i] = m.sum()
        pre[i] = bool(gt.get('already_detect', False))
        r = np.packbits(m, axis=1, bitorder='little')
        rows.append(r.ravel())
        nbytes += r.size
    bits = np.concatenate(rows) if rows else np.zeros(0, np.uint8)
    return bounds, offsets, bits, areas, pre


def sds_class_predictions(det_file, seg_file, num_images):
    """voc_eval_sds's ranking of one class's predictions without its per-prediction loop: -> boxes float64 [P,4], masks uint8
    [P, MASK_SIZE^2] and image indices [P] in the order of np.argsort(-score) over the same float64 score column."""
    with open(det_file, 'rb') as f:
        boxes_pkl = pickle.load(f)
    with open(seg_file, 'rb') as f:
        masks_pkl = pickle.load(f)
    S = cfg.MASK_SIZE
    boxes, masks, image = [np.zeros((0, 5))], [np.zeros((0, S * S), np.uint8)], []
    for image_ind in range(num_images):
        n = len(boxes_pkl[image_ind])
        if n == 0:
            continue
        boxes.append(np.asarray(boxes_pkl[image_ind], dtype=np.float64).reshape(n, 5))
        m = np.asarray(masks_pkl[image_ind])[:n].reshape(n, S * S)
        m8 = m.astype(np.uint8)
        if m.dtype != bool and not np.array_equal(m8, m):
            raise ValueError('masks of image %d are not 0/1 (the _seg.pkl masks are binarised)' % image_ind)
        masks.append(m8)
        image.append(np.full(n, image_ind, np.int64))
    new_boxes = np.concatenate(boxes)
    keep_inds = np.argsort(-new_boxes[:, -1])
    image = np.concatenate(image) if image else np.zeros(0, np.int64)
    return new_boxes[keep_inds, :4], np.concatenate(masks)[keep_inds], image[keep_inds]


def sds_match(best_gt, ov, ov_thresh, pre_matched=None):
    """voc_eval_sds's greedy matching at one threshold, vectorised: a prediction (in ranked order) is a true positive iff its
    best overlap is >= ov_thresh and it is the first such prediction of its best GT (which was not matched before).  Every
    other prediction is a false positive.  -> tp, fp float64 [P]."""
    hit = np.nonzero((best_gt >= 0) & (ov >= ov_thresh))[0]
    g = best_gt[hit]
    _, first = np.unique(g, return_index=True)
    tp_idx = hit[first]
    if pre_matched is not None:
        tp_idx = tp_idx[~pre_matched[g[first]]]
    tp = np.zeros(len(best_gt))
    tp[tp_idx] = 1
    return tp, 1 - tp


def sds_device_inputs(det_path, seg_path, image_names, class_names, cache_dir):
    """Everything mnc_sds_best_overlap needs for all classes at once: the predictions of every class (each ranked as by
    voc_eval_sds) one after the other, and the GT instances of every (class, image) pair that has predictions packed with
    pack_sds_gt.  det_path / seg_path are formatted with the class name.  -> dict."""
    classes = [c for c in class_names if c != '__background__']
    boxes, masks, begin, end, gts, slices, num_pos = [], [], [], [], [], [], []
    lo = 0
    for cls in classes:
        b, m, img = sds_class_predictions(det_path.format(cls), seg_path.format(cls), len(image_names))
        with open(os.path.join(cache_dir, cls + '_mask_gt.pkl'), 'rb') as f:
            gt_pkl = pickle.load(f)
        num_pos.append(sum(len(val) for val in gt_pkl.values()))
        rb = np.zeros(len(image_names), np.int32)
        re = np.zeros(len(image_names), np.int32)
        ranges = {}                          # one GT range per image name (a repeated name shares its instances)
        for ii in np.unique(img):
            name = image_names[ii]
            if name not in gt_pkl:
                continue
            if name not in ranges:
                ranges[name] = (len(gts), len(gts) + len(gt_pkl[name]))
                gts.extend(gt_pkl[name])
            rb[ii], re[ii] = ranges[name]
        boxes.append(b)
        masks.append(m)
        begin.append(rb[img])
        end.append(re[img])
        slices.append((lo, lo + len(b)))
        lo += len(b)
    bounds, offsets, bits, areas, pre = pack_sds_gt(gts)
    return {'classes': classes, 'boxes': np.concatenate(boxes), 'masks': np.concatenate(masks),
            'gt_begin': np.concatenate(begin), 'gt_end': np.concatenate(end), 'gt_bounds': bounds, 'gt_offsets': offsets,
            'gt_bits': bits, 'gt_areas': areas, 'gt_pre': pre, 'gt_dicts': gts, 'slices': slices, 'num_pos': num_pos}


def voc_eval_sds_device(det_path, seg_path, devkit_path, image_list, class_names, cache_dir, ov_threshs=(0.5, 0.7),
                        device_id=None):
    """voc_eval_sds for every class and every threshold of ov_threshs with ONE device call (mnc_sds_best_overlap) for the
    pixel counting; the APs are those of voc_eval_sds, bit for bit.  det_path / seg_path: the per-class result files with
    '{}' for the class name (e.g. output_dir + '/{}_det.pkl').  -> {thresh: [AP of each class but __background__]}."""
    with open(image_list, 'r') as f:
        image_names = [x.strip() for x in f.readlines()]
    check_voc_sds_cache(cache_dir, devkit_path, image_names, class_names)
    d = sds_device_inputs(det_path, seg_path, image_names, class_names, cache_dir)
    best_gt, inter, union = sds_best_overlap(d['boxes'], d['masks'], d['gt_begin'], d['gt_end'], d['gt_bounds'],
                                             d['gt_offsets'], d['gt_bits'], d['gt_areas'], cfg.BINARIZE_THRESH,
                                             cfg.GPU_ID if device_id is None else device_id)
    # mask_overlap's float(inter) / float(union), 0 for union < 1 (and for -1, whose union is 0)
    ov = np.zeros(len(best_gt))
    ok = union >= 1
    ov[ok] = inter[ok] / union[ok]
    result = {}
    for thr in ov_threshs:
        aps = []
        for (lo, hi), num_pos in zip(d['slices'], d['num_pos']):
            tp, fp = sds_match(best_gt[lo:hi], ov[lo:hi], thr, d['gt_pre'])
            fp = np.cumsum(fp)
            tp = np.cumsum(tp)
            rec = tp / float(num_pos)
            prec = tp / np.maximum(fp + tp, np.finfo(np.float64).eps)
            aps.append(voc_ap(rec, prec, True))
        result[thr] = aps
    return result
