"""Deterministic inputs of the box-detection AP golden (box_eval_golden.json, written by
make_box_eval_golden.py from the reference's tools/eval_det.py).

det_cases(): name -> (pred_all, gt_all) in eval_det's layout ({img: [(cls, box, score)]} /
{img: [(cls, box)]}), each built around one rule of the matching.  Confidence ties appear only where
every tie order gives the same result (the generator asserts that).
scene_cases(): name -> small scans (coords, pred masks, semantic and instance labels) whose boxes the
reference's __main__ forms with coords[mask].min(0) / .max(0).
"""
import numpy as np

THRESHOLDS = (0.25, 0.5)
CLASSES = ['cabinet', 'bed', 'chair', 'sofa', 'table']


def B(*v):
    return np.array(v, np.float64)


def det_cases():
    c = {}
    # disjoint, touching (min_max == max_min on one axis -> 0) and single-point boxes
    c['disjoint_touching_point'] = (
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1), 0.9), ('chair', B(1, 0, 0, 2, 1, 1), 0.8),
                ('chair', B(5, 5, 5, 5, 5, 5), 0.7), ('chair', B(10, 10, 10, 11, 11, 11), 0.6)]},
        {'s0': [('chair', B(1, 0, 0, 3, 1, 1)), ('chair', B(5, 5, 5, 5, 5, 5)), ('chair', B(0, 0, 0, 1, 1, 1))]})
    # two detections of one GT: the second is a false positive
    c['duplicate'] = (
        {'s0': [('bed', B(0, 0, 0, 2, 2, 2), 0.9), ('bed', B(0.1, 0, 0, 2, 2, 2), 0.8)]},
        {'s0': [('bed', B(0, 0, 0, 2, 2, 2))]})
    # the second detection's best GT is taken, its second best is free: still a false positive
    c['best_taken_second_free'] = (
        {'s0': [('sofa', B(0, 0, 0, 2, 2, 2), 0.9), ('sofa', B(0.2, 0, 0, 2.2, 2, 2), 0.8)]},
        {'s0': [('sofa', B(0, 0, 0, 2, 2, 2)), ('sofa', B(1.0, 0, 0, 3, 2, 2))]})
    # exact IoU tie between two GTs: the first one is jmax
    c['iou_tie'] = (
        {'s0': [('table', B(1, 0, 0, 3, 1, 1), 0.9), ('table', B(0, 0, 0, 2, 1, 1), 0.5)]},
        {'s0': [('table', B(0, 0, 0, 2, 1, 1)), ('table', B(2, 0, 0, 4, 1, 1))]})
    # IoU exactly 0.5 and exactly 0.25 (ovmax > ovthresh is strict)
    c['at_threshold'] = (
        {'s0': [('cabinet', B(0, 0, 0, 1, 1, 1), 0.9)], 's1': [('cabinet', B(0, 0, 0, 1, 1, 1), 0.8)]},
        {'s0': [('cabinet', B(0, 0, 0, 2, 1, 1))], 's1': [('cabinet', B(0, 0, 0, 4, 1, 1))]})
    # a class with predictions and no GT anywhere (npos = 0), next to a normal one
    c['npos_zero'] = (
        {'s0': [('bed', B(0, 0, 0, 1, 1, 1), 0.9), ('chair', B(0, 0, 0, 1, 1, 1), 0.4)]},
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1))]})
    # a GT class without predictions: eval_det raises KeyError, eval_sphere reports 0
    c['gt_class_without_pred'] = (
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1), 0.9)]},
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1)), ('sofa', B(3, 3, 3, 4, 4, 4))]})
    # images with predictions and no GT (of that class or at all)
    c['pred_images_without_gt'] = (
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1), 0.9)], 's1': [('chair', B(0, 0, 0, 1, 1, 1), 0.95)],
         's2': [('chair', B(0, 0, 0, 1, 1, 1), 0.3), ('table', B(0, 0, 0, 1, 1, 1), 0.6)]},
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1))], 's2': [('table', B(0, 0, 0, 1, 1, 2))]})
    # no predictions at all
    c['empty_pred'] = ({}, {'s0': [('chair', B(0, 0, 0, 1, 1, 1))]})
    c['empty_pred_no_gt'] = ({}, {})
    # confidence ties whose order cannot matter: tied detections are all TPs or all FPs
    c['confidence_ties'] = (
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1), 0.5), ('chair', B(5, 5, 5, 6, 6, 6), 0.5),
                ('chair', B(9, 9, 9, 9.5, 9.5, 9.5), 0.25), ('chair', B(20, 0, 0, 21, 1, 1), 0.25)],
         's1': [('chair', B(0, 0, 0, 1, 1, 1), 0.5), ('chair', B(0, 0, 0, 1.1, 1, 1), 0.1)]},
        {'s0': [('chair', B(0, 0, 0, 1, 1, 1)), ('chair', B(5, 5, 5, 6, 6, 6))],
         's1': [('chair', B(0, 0, 0, 1, 1, 1)), ('chair', B(30, 0, 0, 31, 1, 1))]})
    c['random'] = random_case(7, n_img=4, n_cls=3, n_gt=6, n_det=10)
    return c


def random_case(seed, n_img, n_cls, n_gt, n_det, classes=CLASSES, jitter=0.3):
    """GT boxes per image and jittered detections around them (plus strays), %.4f confidences"""
    rng = np.random.default_rng(seed)
    pred_all, gt_all = {}, {}
    for i in range(n_img):
        img = f'scene{i:04d}_00'
        lo = rng.uniform(0, 8, (n_gt, 3))
        gts = np.concatenate([lo, lo + rng.uniform(0.3, 2, (n_gt, 3))], 1)
        gcls = rng.integers(0, n_cls, n_gt)
        gt_all[img] = [(classes[k], g) for k, g in zip(gcls, gts)]
        preds = []
        for _ in range(n_det):
            j = rng.integers(0, n_gt)
            box = gts[j] + rng.normal(0, jitter, 6)
            box[3:] = np.maximum(box[3:], box[:3] + 0.05)
            k = gcls[j] if rng.uniform() < 0.8 else rng.integers(0, n_cls)
            preds.append((classes[k], box, float(f'{rng.uniform():.4f}')))
        pred_all[img] = preds
    return pred_all, gt_all


def iou_pairs():
    """(box_a, box_b) for get_iou"""
    return [(B(0, 0, 0, 1, 1, 1), B(0.5, 0.5, 0.5, 1.5, 1.5, 1.5)), (B(0, 0, 0, 1, 1, 1), B(1, 0, 0, 2, 1, 1)),
            (B(0, 0, 0, 1, 1, 1), B(2, 2, 2, 3, 3, 3)), (B(1, 1, 1, 1, 1, 1), B(1, 1, 1, 1, 1, 1)),
            (B(-3.25, -1, 0.1, 0.3, 2.7, 1.9), B(-1.1, -2, 0, 0.7, 0.4, 2.2)),
            (B(0, 0, 0, 2, 1, 1), B(0, 0, 0, 1, 1, 1)), (B(0.1, 0.2, 0.3, 0.7, 0.9, 1.3), B(0, 0, 0, 1, 1, 1))]


def voc_inputs():
    """(rec, prec) pairs for voc_ap"""
    return [(np.array([0.5, 0.5, 1.0]), np.array([1.0, 0.5, 0.6666666666666666])),
            (np.array([0.0, 0.25, 0.25, 0.5, 0.75]), np.array([0.0, 0.5, 0.3333333333333333, 0.5, 0.6])),
            (np.zeros(0), np.zeros(0)),
            (np.array([np.nan, np.nan]), np.array([1.0, 0.5])),
            (np.array([np.inf, np.inf]), np.array([1.0, 1.0]))]


def scene_cases():
    """name -> (coords, masks, semantic, instance, label_ids, confs) per scan lists"""
    out = {}
    for name, seed, n_scans, dtype in (('f32', 3, 3, np.float32), ('f64_negative', 4, 2, np.float64)):
        rng = np.random.default_rng(seed)
        coords, masks, sems, insts, labels, confs = [], [], [], [], [], []
        for s in range(n_scans):
            n = 400 + 50 * s
            xyz = rng.normal(0, 2, (n, 3)).astype(dtype)
            if name == 'f64_negative':
                xyz -= 5
            k = 6
            inst = rng.integers(0, k, n).astype(np.int64)
            inst[rng.uniform(size=n) < 0.2] = -100
            inst[:k] = np.arange(k)                      # every instance id has a point
            cls_of = rng.integers(0, 2 + len(CLASSES), k)
            sem = cls_of[np.maximum(inst, 0)].astype(np.int64)
            sem[inst < 0] = rng.integers(0, 2, int((inst < 0).sum()))
            sem[rng.uniform(size=n) < 0.05] = -100
            ms, ls, cs = [], [], []
            for p in range(8):
                base = inst == rng.integers(0, k)
                m = (base ^ (rng.uniform(size=n) < 0.05)).astype(np.int64)
                m[rng.integers(0, n)] = 1
                ms.append(m)
                ls.append(int(rng.integers(1, len(CLASSES) + 1)))
                cs.append(float(f'{rng.uniform():.4f}'))
            coords.append(xyz)
            masks.append(ms)
            sems.append(sem)
            insts.append(inst)
            labels.append(ls)
            confs.append(cs)
        out[name] = (coords, masks, sems, insts, labels, confs)
    return out


VALID_CLASS_IDS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]   # ScanNet nyu ids


def write_out_tree(root, name='f32'):
    """a scene case as tools/test.py --out and the dataset leave it: <root>/val/<scan>_inst_nostuff.pth
    and <root>/results/pred_instance/{<scan>.txt, predicted_masks/<scan>_<i>.txt} (CLASSES are the first
    names of the ScanNet list, so the nyu ids map back to them) -> (data_path, results_path)"""
    import os
    import torch
    coords, masks, sems, insts, labels, confs = scene_cases()[name]
    data, results = os.path.join(root, 'val'), os.path.join(root, 'results')
    os.makedirs(data, exist_ok=True)
    os.makedirs(os.path.join(results, 'pred_instance', 'predicted_masks'), exist_ok=True)
    for s in range(len(coords)):
        scan = f'scene{s:04d}_00'
        rgb = np.zeros_like(coords[s])
        torch.save((coords[s], rgb, sems[s].astype(np.float64), insts[s].astype(np.float64)),
                   os.path.join(data, scan + '_inst_nostuff.pth'))
        with open(os.path.join(results, 'pred_instance', scan + '.txt'), 'w') as f:
            for i, (m, lab, c) in enumerate(zip(masks[s], labels[s], confs[s])):
                f.write(f'predicted_masks/{scan}_{i:03d}.txt {VALID_CLASS_IDS[lab - 1]} {c:.4f}\n')
                np.savetxt(os.path.join(results, 'pred_instance', 'predicted_masks', f'{scan}_{i:03d}.txt'), m,
                           fmt='%d')
    return data, results
