"""Axis-aligned box AP of saved instance predictions on ScanNet v2 ("Bounding box evaluation"): a
drop-in for the reference's tools/eval_det.py on the files tools/test.py --out writes.

Reads <results>/pred_instance/<scan>.txt (lines "predicted_masks/<scan>_<i>.txt <nyu id> <score>"),
the masks under <results>/pred_instance/predicted_masks/ (one value per point, nonzero = in) and
<data>/<scan>_inst_nostuff.pth (coords, colors, semantic labels, instance labels), forms the boxes
and scores them with eval_sphere for every --iou threshold (one IoU pass for all of them).

    python tools/eval_det.py --data-path dataset/scannetv2/val --results-path results --iou 0.25 0.5

With --boxes obb the masks and GT instances get yaw-oriented boxes (--yaw-steps directions) and are
scored by the oriented IoU, --mode 3d (volumes) or bev (the rectangles in the xy plane); the default
--boxes aabb is the reference's evaluation.
"""
import argparse
import glob
import os.path as osp
import sys

import numpy as np
import torch

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
from softgroup_amd.evaluation import evaluate_box_ap  # noqa: E402

CLASS_LABELS = [
    'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window', 'bookshelf', 'picture', 'counter', 'desk',
    'curtain', 'refrigerator', 'shower curtain', 'toilet', 'sink', 'bathtub', 'otherfurniture'
]
VALID_CLASS_IDS = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]


def read_mask(path):
    """one integer per line -> bool mask (any nonzero value is in)"""
    with open(path, 'rb') as f:
        return np.array(f.read().split(), dtype=np.int64) != 0


def load_scan(data_path, results_path, instance_path):
    scan = osp.basename(instance_path)[:-4]
    gt_path = osp.join(data_path, scan + '_inst_nostuff.pth')
    assert osp.isfile(gt_path), gt_path
    coords, _, semantic_label, instance_label = torch.load(gt_path, weights_only=False)
    preds = []
    with open(instance_path) as f:
        for line in f:
            fields = line.split()
            if not fields:
                continue
            mask_path, label, score = fields
            mask = read_mask(osp.join(results_path, 'pred_instance', mask_path))
            preds.append(dict(scan_id=scan, label_id=VALID_CLASS_IDS.index(int(label)) + 1, conf=float(score),
                              pred_mask=mask))
    return scan, preds, np.asarray(coords), np.asarray(semantic_label), np.asarray(instance_label)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--data-path', default='./dataset/scannetv2/val/')
    ap.add_argument('--results-path', default='./results', help='the --out directory of tools/test.py')
    ap.add_argument('--iou', type=float, nargs='+', default=[0.25], help='IoU thresholds')
    ap.add_argument('--use-07-metric', action='store_true', help='VOC07 11-point AP')
    ap.add_argument('--device', default=None, help="'cuda', 'cpu' or unset (the GPU when there is one)")
    ap.add_argument('--boxes', choices=['aabb', 'obb'], default='aabb',
                    help="'aabb': the reference's axis-aligned boxes; 'obb': yaw-oriented boxes and their IoU")
    ap.add_argument('--mode', choices=['3d', 'bev'], default='3d', help="with --boxes obb: volume or bird's-eye IoU")
    ap.add_argument('--yaw-steps', type=int, default=90, help='with --boxes obb: directions of the yaw sweep')
    args = ap.parse_args(argv)
    paths = sorted(glob.glob(osp.join(args.results_path, 'pred_instance', '*.txt')))
    preds, coords, sems, insts = [], [], [], []
    for p in paths:
        scan, pr, c, s, i = load_scan(args.data_path, args.results_path, p)
        print('Processing', scan)
        preds.append(pr)
        coords.append(c)
        sems.append(s)
        insts.append(i)
    print('Evaluating...')
    res = evaluate_box_ap(preds, coords, sems, insts, CLASS_LABELS, iou_thresholds=args.iou,
                          use_07_metric=args.use_07_metric, device=args.device, boxes=args.boxes, mode=args.mode,
                          yaw_steps=args.yaw_steps)
    for t in args.iou:
        print(f'IoU threshold: {t}')
        print('mAP:', res[t]['mAP'])
    return res


if __name__ == '__main__':
    main()
