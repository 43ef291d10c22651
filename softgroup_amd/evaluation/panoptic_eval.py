"""Panoptic quality for SemanticKITTI (``eval_tasks: ['panoptic']``).  Same interface and
results as the reference's ``PanopticEval`` (softgroup/evaluation/panoptic_eval.py:7-264, itself
after the semantic-kitti-api's eval_np.py): ``evaluate`` returns the same 10-tuple and prints the
same table, ``evaluate_single`` returns the same 7 per-scan arrays.

On the GPU all scans of a chunk (cut at scan boundaries by ``max_chunk_points``) go to the device
once.  ``sg_eval_class_tally`` counts seen / positive / correct, ``sg_eval_panoptic_segments`` counts
the pred segments, gt segments and their intersections in hash tables, computes the IoU of every
distinct pair and returns the TP rows (scan, class, combo, I, U) plus the FP / FN counts.  The host
sorts the few TP rows by (scan, class, combo) and forms ``pan_iou`` with the reference's own numpy
reductions, so every figure equals the numpy path's to the bit.  Inputs the kernels cannot represent
exactly (float labels, ids outside 32 bits, an ``offset`` other than 2**32, more than
SG_EVAL_MAX_CLASSES classes) take the numpy path.

``getPQ`` is not provided: the reference's reads ``self.include``, which it never sets, so it cannot
run there either.
"""
import numpy as np

from .point_wise_eval import (_BAD_INST, _BAD_PRED, MAX_CLASSES, _is_int, chunks, host, label_kind, stage,
                              use_device)


class PanopticEval:

    def __init__(self, thing_classes, stuff_classes, offset=2**32, min_points=50, ignore_label=-100, *,
                 device=None, max_chunk_points=1 << 21):
        self.thing_classes = thing_classes
        self.stuff_classes = stuff_classes
        self.classes = stuff_classes + thing_classes
        self.n_classes = len(self.classes)
        self.ignore_label = ignore_label
        self.offset = offset
        self.min_points = min_points
        self.eps = 1e-15
        self.device = device                      # None: GPU when available
        self.max_chunk_points = max_chunk_points  # bounds the device memory of one launch set

    # ------------------------------------------------------------------ numpy path
    def _single_numpy(self, panoptic_pred, y_sem_row, y_inst_row):
        n = self.n_classes
        pan_tp = np.zeros(n, dtype=np.int64)
        pan_iou = np.zeros(n, dtype=np.double)
        pan_fp = np.zeros(n, dtype=np.int64)
        pan_fn = np.zeros(n, dtype=np.int64)
        seen = np.zeros(n, dtype=np.int64)
        correct = np.zeros(n, dtype=np.int64)
        positive = np.zeros(n, dtype=np.int64)

        pred = host(panoptic_pred)
        y_sem = host(y_sem_row)
        y_inst = host(y_inst_row).copy()          # the inputs stay as they are
        x_sem = pred & 0xFFFF
        # x_inst = pred + 1: the WHOLE 32-bit value with its class bits, so all stuff points of a
        # class (id 0) are one segment
        x_inst = pred + 1
        # y_inst: ignore -> -1, then + 2: ignored-instance gt points of a class form segment 1;
        # labels below -1 give y <= 0 and are no segment
        y_inst[y_inst == self.ignore_label] = -1
        y_inst = y_inst + 1
        y_inst = y_inst + 1
        # only the points with y_sem != ignore count
        keep = y_sem != self.ignore_label
        x_sem, y_sem, x_inst, y_inst = x_sem[keep], y_sem[keep], x_inst[keep], y_inst[keep]

        for cl in range(n):
            xm, ym = x_sem == cl, y_sem == cl
            seen[cl] = ym.sum()
            correct[cl] = (ym & xm).sum()
            positive[cl] = xm.sum()
            x_in = x_inst * xm.astype(np.int64)
            y_in = y_inst * ym.astype(np.int64)
            u_pred, n_pred = np.unique(x_in[x_in > 0], return_counts=True)
            u_gt, n_gt = np.unique(y_in[y_in > 0], return_counts=True)
            both = (x_in > 0) & (y_in > 0)
            combo, inter = np.unique(x_in[both] + self.offset * y_in[both], return_counts=True)
            g = np.searchsorted(u_gt, combo // self.offset)
            p = np.searchsorted(u_pred, combo % self.offset)
            union = n_gt[g] + n_pred[p] - inter
            # IoU in float64; a TP is IoU > 0.5, strictly
            ious = inter.astype(np.float64) / union.astype(np.float64)
            tp = ious > 0.5
            pan_tp[cl] += np.sum(tp)
            # np.sum of the TP IoUs in ascending x + offset * y order
            pan_iou[cl] += np.sum(ious[tp])
            m_gt = np.zeros(len(u_gt), bool)
            m_pred = np.zeros(len(u_pred), bool)
            m_gt[g[tp]] = True
            m_pred[p[tp]] = True
            # min_points only applies to FN / FP, never to the IoU
            pan_fn[cl] += np.sum((n_gt >= self.min_points) & ~m_gt)
            pan_fp[cl] += np.sum((n_pred >= self.min_points) & ~m_pred)
        return pan_tp, pan_iou, pan_fp, pan_fn, seen, correct, positive

    # ------------------------------------------------------------------ device path
    def _device_ok(self, preds, sems, insts):
        return (self.offset == 2**32 and _is_int(self.min_points) and _is_int(self.ignore_label)
                and -2**63 <= int(self.ignore_label) < 2**63 and 1 <= self.n_classes <= MAX_CLASSES
                and len(preds) == len(sems) == len(insts) and len(preds) > 0
                and None not in (label_kind(preds), label_kind(sems), label_kind(insts))
                and all(int(a.shape[0]) == int(b.shape[0]) == int(c.shape[0]) < 2**30
                        for a, b, c in zip(preds, sems, insts)))

    def _per_scan_device(self, preds, sems, insts):
        """-> pan_tp, pan_iou [n_scans, n_classes] and the summed fp, fn, seen, correct, positive;
        None when an input cannot be packed exactly"""
        import torch
        from .. import _lib as L
        n, n_scans = self.n_classes, len(preds)
        pk, sk, ik = label_kind(preds), label_kind(sems), label_kind(insts)
        sizes = [int(a.shape[0]) for a in preds]
        dev = torch.device('cuda' if self.device is None else self.device)
        pan_tp = np.zeros((n_scans, n), np.int64)
        pan_iou = np.zeros((n_scans, n), np.double)
        totals = np.zeros(5 * n, np.int64)                    # seen | positive | correct | fp | fn
        with torch.cuda.device(dev):
            # one block read back per chunk: flags, TP count, tallies, fp, fn
            head = torch.zeros(2 + 5 * n, dtype=torch.int64, device=dev)
            for a, b in chunks(sizes, self.max_chunk_points):
                npts = sum(sizes[a:b])
                pred, sem, inst = (stage(preds[a:b], pk, dev), stage(sems[a:b], sk, dev),
                                   stage(insts[a:b], ik, dev))
                off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes[a:b])]).astype(np.int64)).to(dev)
                tp_rows = torch.empty(max(4 * npts, 4), dtype=torch.int64, device=dev)
                ws = L.workspace(max(L.lib().sg_eval_panoptic_workspace_bytes(npts),
                                     L.lib().sg_eval_tally_workspace_bytes(npts)), dev)
                head.zero_()
                base, flags = head.data_ptr(), head.data_ptr()
                L.check(L.lib().sg_eval_class_tally(
                    L.ptr(pred), pk, L.ptr(sem), sk, npts, int(self.ignore_label), 1, n, base + 16, None, 0,
                    None, None, None, None, flags, L.ptr(ws), ws.numel(), L.stream()), 'sg_eval_class_tally')
                L.check(L.lib().sg_eval_panoptic_segments(
                    L.ptr(pred), pk, L.ptr(sem), sk, L.ptr(inst), ik, L.ptr(off), b - a, npts,
                    int(self.ignore_label), n, int(self.min_points), base + 16 + 8 * 3 * n, L.ptr(tp_rows),
                    base + 8, flags, L.ptr(ws), ws.numel(), L.stream()), 'sg_eval_panoptic_segments')
                h = head.cpu().numpy()
                # (a gt class outside [0, n_classes) just counts nowhere, as in the reference)
                if int(h[0]) & (_BAD_PRED | _BAD_INST):
                    return None
                totals += h[2:]
                rows = tp_rows[:4 * int(h[1])].cpu().numpy().reshape(-1, 4)
                if len(rows):
                    scan = (rows[:, 0] >> 16) + a
                    cl = rows[:, 0] & 0xFFFF
                    order = np.lexsort((rows[:, 1], cl, scan))          # (scan, class, combo)
                    scan, cl, rows = scan[order], cl[order], rows[order]
                    ious = rows[:, 2].astype(np.float64) / rows[:, 3].astype(np.float64)
                    key = scan * n + cl
                    starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
                    for s, e in zip(starts, np.append(starts[1:], len(key))):
                        pan_tp[scan[s], cl[s]] = e - s
                        # the same np.sum over the same ascending-combo vector as the numpy path
                        pan_iou[scan[s], cl[s]] = np.sum(ious[s:e])
        seen, positive, correct, fp, fn = totals.reshape(5, n)
        return pan_tp, pan_iou, fp, fn, seen, correct, positive

    # ------------------------------------------------------------------ public interface
    def evaluate_single(self, panoptic_pred, y_sem_row, y_inst_row):
        args = ([panoptic_pred], [y_sem_row], [y_inst_row])
        if use_device(self.device) and self._device_ok(*args):
            r = self._per_scan_device(*args)
            if r is not None:
                pan_tp, pan_iou, fp, fn, seen, correct, positive = r
                return pan_tp[0], pan_iou[0], fp, fn, seen, correct, positive
        return self._single_numpy(panoptic_pred, y_sem_row, y_inst_row)

    def _accumulate(self, panoptic_preds, sem_labels, inst_labels):
        args = (list(panoptic_preds), list(sem_labels), list(inst_labels))
        if use_device(self.device) and self._device_ok(*args):
            r = self._per_scan_device(*args)
            if r is not None:
                pan_tp, pan_iou, pan_fp, pan_fn, seen, correct, positive = r
                return pan_tp.sum(axis=0), pan_iou.sum(axis=0), pan_fp, pan_fn, seen, correct, positive
        results = [self._single_numpy(*a) for a in zip(*args)]
        # across scans: np.stack(...).sum(axis=0), sequential over the scans
        return tuple(np.stack(r).sum(axis=0) for r in zip(*results))

    def evaluate(self, panoptic_preds, sem_labels, inst_labels):
        pan_tp, pan_iou, pan_fp, pan_fn, seen, correct, positive = self._accumulate(
            panoptic_preds, sem_labels, inst_labels)
        n_stuff = len(self.stuff_classes)
        iou_all = correct / np.maximum((seen + positive - correct).astype(np.double), self.eps)
        sq_all = pan_iou.astype(np.double) / np.maximum(pan_tp.astype(np.double), self.eps)
        rq_all = pan_tp.astype(np.double) / np.maximum(
            pan_tp.astype(np.double) + 0.5 * pan_fp.astype(np.double) + 0.5 * pan_fn.astype(np.double), self.eps)
        pq_all = sq_all * rq_all
        # PQ-dagger: the stuff classes take their IoU in place of PQ
        pq_dagger_all = pq_all.copy()
        pq_dagger_all[:n_stuff] = iou_all[:n_stuff]
        pq_all *= 100
        sq_all *= 100
        rq_all *= 100
        iou_all *= 100
        pq_dagger_all *= 100
        SQ, RQ, PQ = sq_all.mean(), rq_all.mean(), pq_all.mean()
        PQ_dagger, IoU = pq_dagger_all.mean(), iou_all.mean()
        self.print_results(PQ, PQ_dagger, SQ, RQ, IoU, pq_all, pq_dagger_all, sq_all, rq_all, iou_all)
        return PQ, PQ_dagger, SQ, RQ, IoU, pq_all, pq_dagger_all, sq_all, rq_all, iou_all

    def print_results(self, PQ, PQ_dagger, SQ, RQ, IoU, pq_all, pq_dagger_all, sq_all, rq_all, iou_all):
        n_stuff, n_thing = len(self.stuff_classes), len(self.thing_classes)
        stuff = [np.full(pq_all.shape, np.nan) for _ in range(3)]
        thing = [np.full(pq_all.shape, np.nan) for _ in range(3)]
        for dst, src in zip(stuff, (pq_all, rq_all, sq_all)):
            dst[:n_stuff] = src[:n_stuff]
        for dst, src in zip(thing, (pq_all, rq_all, sq_all)):
            dst[-n_thing:] = src[-n_thing:]       # (with no thing class, -0: is the whole row, as there)
        width = 81
        print()
        print('#' * width)
        cols = ('PQ', 'PQ*', 'RQ', 'SQ', 'PQ_t', 'RQ_t', 'SQ_t', 'PQ_s', 'RQ_s', 'SQ_s', 'mIoU')
        print('{:<14}'.format('what') + ':' + ''.join('{:>6}'.format(c) for c in cols))
        print('#' * width)
        for i in range(self.n_classes):
            vals = (pq_all[i], pq_dagger_all[i], rq_all[i], sq_all[i], thing[0][i], thing[1][i], thing[2][i],
                    stuff[0][i], stuff[1][i], stuff[2][i], iou_all[i])
            print('{:<14}'.format(self.classes[i]) + ':' + ''.join('{:>6.1f}'.format(v) for v in vals))
        print('-' * width)
        vals = (PQ, PQ_dagger, RQ, SQ) + tuple(np.nanmean(a) for a in thing + stuff) + (IoU,)
        print('{:<14}'.format('average') + ':' + ''.join('{:>6.1f}'.format(v) for v in vals))
        print('#' * width)
