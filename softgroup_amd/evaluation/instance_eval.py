"""Instance-segmentation evaluation (AP / AP50 / AP25 / recall), the step right AFTER the hot path
(SURVEY 8f-3).  Same interface and results as the reference's ``ScanNetEval``
(softgroup/evaluation/instance_eval.py: ``evaluate(pred_list, gt_list)`` -> dict of averages,
``print_results``, ``write_result_file``), which follows the ScanNet benchmark's
evaluate_semantic_instance.py.

What differs is how a scan's predictions are associated with its ground truth.  The reference
decodes every RLE mask to a dense 0/1 array and, for every (prediction, GT instance) pair of equal
class, counts ``logical_and`` over all N points, in a multiprocessing pool (:228-309, 375-385).
Here the masks stay runs: all runs of a scan go to the GPU once and ``sg_eval_intersections``
visits every mask point exactly once, producing the whole prediction x GT count matrix (plus the
"void" column) -- O(total mask points) instead of O(nPred * nGT * N).  Without a GPU the same
matrix comes from ``numpy.add.at`` (the evaluator is also used in CPU-only tooling).

The matching / precision-recall logic is kept operation for operation (greedy assignment in
prediction order, the duplicate-match rule, ignore proportions from void and small instances,
unique-threshold PR curve with the [-0.5, 0, 0.5] step kernel), so the averages equal the
reference's to the last bit; tests/golden/eval_golden.json pins that against the reference's own
evaluator.

``backend='device'`` (opt-in: ``evaluate(..., backend='device')``, or ``reset()`` / ``update(preds, gts)``
per scan / ``compute()``) moves the rest to the GPU as well (csrc/inst_eval.hip).  Stages:

1. RLE text -> runs (``sg_inst_rle_parse``): the host only joins a scan's ``counts`` strings; dense-array
   masks keep using ``_runs_of``.
2. association, per scan (``sg_inst_scan_update``): GT table from a histogram of the ids (ascending id,
   ``np.unique``'s order), count matrix with the void column, pair records (gt, pred, inter, iou) in both
   orders the matcher walks.
3. matching, per scan in the same call: one work item per (label, threshold) -- the reference's
   ``visited`` keys carry the scan id, so the greedy walk is sequential only inside (scan, label,
   threshold) -- count walk, scan, emit walk; (score, true flag) examples, hard false negatives and the
   has_gt / has_pred flags are appended to a device-resident accumulator.
4. curves, once (``sg_inst_curves``): examples sorted by (segment, order-preserving score key), cumulative
   true count, unique boundaries, precision / recall in double, AP summed in a fixed order.

``update`` copies a scan's inputs through pinned staging and enqueues on the current stream; it reads
nothing back, so the scan's evaluation overlaps the next forward.  ``compute`` reads the example count
and the flag word (24 bytes), launches stage 4 and reads ap / rc [n_labels, 10] back; ``compute_averages``
is the host's.  ``last_backend`` / ``last_fallback`` say what ran: duplicate scan ids, a GT id outside
[0, 2**31), a non-finite confidence, more than 65 535 scans and the reference's IndexError case hand the
whole evaluation to the host path; an accumulator that proves too small is detected by the kernels
(nothing is truncated silently) and the evaluation is redone with more room from the inputs, which are
kept by reference until ``compute``; malformed RLE text raises ValueError.

``coverage=True`` (or ``dict(iou_thr=0.5, score_thr=0.0)``) adds the columns of the S3DIS tables (ASIS,
PointGroup, HAIS, SoftGroup): mean coverage, size-weighted coverage, and precision / recall at one IoU
threshold.  The reference has no code for them; per scan and evaluated label l they are defined as

  GT instances         the evaluated ids of l, ascending, all sizes
  participating preds  those that take part above (valid label, >= min region size) with conf >= score_thr
  ov_gt(g), ov_pred(p) the best IoU over the participating predictions / the GT instances of l, 0.0 without any
  cov, wcov            (sum_g ov_gt(g)) / n_gt and (sum_g ov_gt(g) * vert(g)) / sum_g vert(g), when n_gt > 0
                       (the scan is then a room of l)
  tp / fp              a participating prediction with ov_pred >= iou_thr / below it
  gt_hit               the GT instances with ov_gt >= iou_thr

and over the scans ``cov[l] = sum of cov / rooms[l]`` (the ASIS protocol: mean per room, then over rooms),
likewise wcov, ``prec[l] = tp / (tp + fp)``, ``rec[l] = gt_hit / n_gt`` (counted on the GT side: with
duplicate predictions the prediction-side count can exceed n_gt), NaN for a zero denominator, and the
``all_*`` figures the nanmean over the labels.  The sums run over ascending GT id and scan after scan, with
a rounded multiply and rounded adds, on the host and in ``sg_inst_scan_coverage`` alike, so both backends
give the same bits.  Without ``coverage`` nothing of this runs and ``avgs`` is what it always was.
"""
import warnings

import numpy as np

_COV_TALLIES = ('rooms', 'n_gt', 'gt_hit', 'tp', 'fp')


def _runs_of(pred_mask, n_points):
    """0-based (starts, lens) of a mask given as RLE dict or array"""
    if isinstance(pred_mask, dict):
        assert int(pred_mask['length']) == n_points
        flat = np.array(pred_mask['counts'].split(), dtype=np.int64) if pred_mask['counts'] else \
            np.zeros(0, np.int64)
        return flat[0::2] - 1, flat[1::2]
    m = np.not_equal(np.asarray(pred_mask), 0)
    assert m.shape[0] == n_points
    edges = np.flatnonzero(np.diff(np.concatenate([[0], m.astype(np.int8), [0]])))
    return edges[0::2], edges[1::2] - edges[0::2]


def _host_gts(gts):
    """gts as the host path takes them (a device tensor comes back to the host)"""
    return gts.detach().cpu().numpy() if hasattr(gts, 'detach') else gts


_INST_BAD_TEXT, _INST_ODD_TOKENS, _INST_RUN_RANGE, _INST_BAD_GT = 1, 2, 4, 8
_INST_OVERFLOW_GT, _INST_OVERFLOW_EX, _INST_NO_EXAMPLES = 16, 32, 64


class _DeviceAccumulator(object):
    """The device backend's state between reset() and compute(): the example accumulator
    (score keys, segment | true flag), the per-(label, threshold) statistics, the flag word -- all on
    the device -- and the scans' inputs by reference, for the two cases in which the evaluation is
    redone: an accumulator that proved too small (redone on the device with more room) and an input
    the kernels do not take (handed to the host path with the reason in `fallback`)."""

    MAX_SCANS = 65535

    def __init__(self, ev):
        import torch
        if not torch.cuda.is_available() or (ev.device is not None and not str(ev.device).startswith('cuda')):
            raise RuntimeError("ScanNetEval backend='device' needs a GPU (device=%r, torch.cuda.is_available()=%s); "
                               "use backend='host'" % (ev.device, torch.cuda.is_available()))
        from .. import _lib as L
        self.L, self.torch, self.ev = L, torch, ev
        self.dev = torch.device('cuda' if ev.device is None else ev.device)
        self.n_classes = len(ev.valid_class_labels)
        self.n_labels = len(ev.eval_class_labels)
        self.n_thr = len(ev.ious)
        self.n_seg = self.n_labels * self.n_thr
        self.thr = np.ascontiguousarray(ev.ious, np.float64)       # the host's float64 values, passed down
        self.min_region = int(ev.min_region_sizes[0])
        self.coverage = ev.coverage
        cap = ev.device_capacity or {}
        self.ex_cap = int(cap.get('examples', 1 << 20))
        self.gt_cap = int(cap.get('gt', 256))
        self.inputs, self.fallback = [], None
        self.scan_ids = set()
        self.grown = 0
        self._alloc()

    def _alloc(self):
        torch = self.torch
        self.ex_key = torch.empty(max(self.ex_cap, 1), dtype=torch.int64, device=self.dev)
        self.ex_meta = torch.empty(max(self.ex_cap, 1), dtype=torch.int32, device=self.dev)
        self.seg_stats = torch.zeros(4 * self.n_seg, dtype=torch.int32, device=self.dev)
        self.meta = torch.zeros(4, dtype=torch.int64, device=self.dev)   # [0] examples, [2] flag word (int32)
        if self.coverage:                                      # doubles [2][n_labels], then int64 [5][n_labels]
            self.cov = torch.zeros(7 * self.n_labels, dtype=torch.int64, device=self.dev)
        self.stream = None

    def _flags_ptr(self):
        return self.meta.data_ptr() + 16

    def _order_streams(self):
        """the accumulator's work stays in order when the caller changes the current stream"""
        cur = self.torch.cuda.current_stream(self.dev)
        if self.stream is not None and self.stream != cur:
            cur.wait_stream(self.stream)
        self.stream = cur

    # -------------------------------------------------------------- one scan
    def update(self, preds, gts):
        self.inputs.append((preds, gts))
        if self.fallback is not None:
            return
        if len(self.inputs) > self.MAX_SCANS:
            self.fallback = 'more than 65535 scans'
            return
        ids = {p.get('scan_id') for p in preds}
        if ids & self.scan_ids:
            self.fallback = 'duplicate scan_id'
            return
        self.scan_ids |= ids
        self._enqueue(preds, gts)

    def _enqueue(self, preds, gts):
        torch, L, ev = self.torch, self.L, self.ev
        if not torch.is_tensor(gts):
            gts = np.asarray(gts)
        n_points = int(gts.shape[0])
        n_pred = len(preds)
        label = np.full(n_pred, -1, np.int32)
        vert = np.zeros(n_pred, np.int32)
        conf = np.zeros(n_pred, np.float64)
        texts, mask_pred, h_start, h_len, h_pred = [], [], [], [], []
        for k, pred in enumerate(preds):
            if ev.use_label:
                if pred['label_id'] not in ev.id2label:
                    continue
                label[k] = int(pred['label_id']) - 1
            else:
                label[k] = 0
            conf[k] = float(pred['conf'])
            m = pred['pred_mask']
            if isinstance(m, dict):
                assert int(m['length']) == n_points
                texts.append(m['counts'])
                mask_pred.append(k)
            else:
                s, n = _runs_of(m, n_points)
                h_start.append(s)
                h_len.append(n)
                h_pred.append(np.full(len(s), k, np.int64))
                vert[k] = int(n.sum())
        if not np.isfinite(conf).all():
            self.fallback = 'non-finite confidence'
            return
        conf += 0.0                                            # -0.0 -> 0.0 (np.unique takes them as equal)
        if n_pred * n_points >= 2 ** 31 or n_points >= 2 ** 31:
            self.fallback = 'more than 2**31 prediction x point pairs in a scan'
            return
        try:
            text = ''.join(texts).encode('ascii')
        except UnicodeEncodeError:
            raise ValueError('malformed RLE text: a character that is neither a digit nor white space')
        n_rle, n_text = len(texts), len(text)
        text_off = np.zeros(n_rle + 1, np.int64)
        text_off[1:] = np.cumsum(np.array([len(t) for t in texts], np.int64))
        n_host = int(sum(len(s) for s in h_start))
        slots_text = int(L.lib().sg_inst_rle_run_slots(n_text, n_rle)) if n_rle else 0
        run_slots = slots_text + n_host

        # everything of the scan in ONE pinned staging buffer and one copy (the caching host allocator keeps
        # the buffer alive until the copy has run): conf | text_off | label | vert | mask_pred | host runs | text
        def up8(x):
            return (x + 7) // 8 * 8
        parts = [conf, text_off, label, vert, np.asarray(mask_pred, np.int32),
                 np.concatenate(h_start).astype(np.int32) if n_host else np.zeros(0, np.int32),
                 np.concatenate(h_len).astype(np.int32) if n_host else np.zeros(0, np.int32),
                 np.concatenate(h_pred).astype(np.int32) if n_host else np.zeros(0, np.int32),
                 np.frombuffer(text, np.uint8)]
        offs, total = [], 0
        for a in parts:
            offs.append(total)
            total += up8(a.nbytes)
        stage = torch.empty(max(total, 8), dtype=torch.uint8, pin_memory=True)
        view = stage.numpy()
        for a, o in zip(parts, offs):
            view[o:o + a.nbytes] = a.view(np.uint8)
        blob = torch.empty(max(total, 8), dtype=torch.uint8, device=self.dev)
        self._order_streams()
        blob.copy_(stage, non_blocking=True)
        base = blob.data_ptr()
        p_conf, p_toff, p_label, p_vert, p_mpred, p_hs, p_hl, p_hp, p_text = (base + o for o in offs)

        if torch.is_tensor(gts):
            d_gts = gts.detach().reshape(-1).to(self.dev, torch.int64, non_blocking=True).contiguous()
        else:
            g = np.asarray(gts).reshape(-1)
            if g.dtype.kind not in 'iu':
                raise TypeError(f'gts must be an integer array, not {g.dtype}')
            pin = torch.empty(max(n_points, 1), dtype=torch.int64, pin_memory=True)
            with np.errstate(over='ignore'):
                pin.numpy()[:n_points] = g                     # (uint64 >= 2**63 wraps negative: flagged on the device)
            d_gts = torch.empty(max(n_points, 1), dtype=torch.int64, device=self.dev)
            d_gts.copy_(pin, non_blocking=True)

        runs = torch.empty((3, max(run_slots, 1)), dtype=torch.int32, device=self.dev)
        if n_host:                                             # runs of dense-array masks follow the text's slots
            src = blob[offs[5]:offs[5] + 4 * n_host].view(torch.int32), \
                blob[offs[6]:offs[6] + 4 * n_host].view(torch.int32), \
                blob[offs[7]:offs[7] + 4 * n_host].view(torch.int32)
            for r in range(3):
                runs[r, slots_text:run_slots].copy_(src[r])
        lib, st = L.lib(), L.stream()
        r_start, r_len, r_pred = (runs.data_ptr() + 4 * r * runs.shape[1] for r in range(3))
        if n_rle:
            L.check(lib.sg_inst_rle_parse(p_text, p_toff, p_mpred, n_rle, n_text, n_points, r_start, r_len, r_pred,
                                          slots_text, p_vert, self._flags_ptr(), st), 'sg_inst_rle_parse')
        ws_bytes = lib.sg_inst_scan_workspace_bytes(n_points, n_pred, run_slots, self.n_classes, self.gt_cap,
                                                    self.n_thr, self.n_labels, None)
        if ws_bytes == 0:
            self.fallback = 'a scan too large for the device tables'
            return
        ws = L.workspace(ws_bytes, self.dev)
        L.check(lib.sg_inst_scan_update(
            d_gts.data_ptr(), n_points, r_start, r_len, r_pred, run_slots, p_label, p_vert, p_conf, n_pred,
            self.n_labels, self.n_classes, self.min_region, self.thr.ctypes.data, self.n_thr, self.gt_cap,
            self.ex_key.data_ptr(), self.ex_meta.data_ptr(), self.ex_cap, self.seg_stats.data_ptr(),
            self.meta.data_ptr(), self._flags_ptr(), ws.data_ptr(), ws_bytes, st), 'sg_inst_scan_update')
        if self.coverage:                                      # over the scan's tables, before ws can be reused
            L.check(lib.sg_inst_scan_coverage(
                n_points, n_pred, run_slots, self.n_classes, self.gt_cap, self.n_thr, self.n_labels, p_label, p_vert,
                p_conf, self.min_region, self.coverage['iou_thr'], self.coverage['score_thr'], self.cov.data_ptr(),
                self.cov.data_ptr() + 16 * self.n_labels, self._flags_ptr(), ws.data_ptr(), ws_bytes, st),
                'sg_inst_scan_coverage')
        # (stage-level tests look at the scan's tables)
        self._last = dict(ws=ws, blob=blob, runs=runs, gts=d_gts, n_points=n_points, n_pred=n_pred,
                          run_slots=run_slots, vert=blob[offs[3]:offs[3] + 4 * n_pred].view(torch.int32))

    # -------------------------------------------------------------- all scans
    def compute(self):
        """-> (ap, rc) as evaluate_matches gives them, or None with self.fallback set"""
        torch, L = self.torch, self.L
        for _ in range(12):
            if self.fallback is not None:
                return None
            self._order_streams()
            meta = self.meta.cpu().numpy()
            n_ex, flags = int(meta[0]), int(meta[2]) & 0xffffffff
            if flags & (_INST_BAD_TEXT | _INST_ODD_TOKENS | _INST_RUN_RANGE):
                what = [t for b, t in ((_INST_BAD_TEXT, 'a byte that is neither a digit nor white space'),
                                       (_INST_ODD_TOKENS, 'an odd number of tokens'),
                                       (_INST_RUN_RANGE, 'a run outside the scan')) if flags & b]
                raise ValueError('malformed RLE text: ' + ', '.join(what))
            if flags & _INST_BAD_GT:
                self.fallback = 'gt id negative or >= 2**31'
                return None
            if not flags & (_INST_OVERFLOW_GT | _INST_OVERFLOW_EX):
                break
            # too small: the whole evaluation again with more room (the inputs were kept by reference)
            if flags & _INST_OVERFLOW_GT:
                self.gt_cap = min(self.gt_cap * 4, self.n_classes * 1000)
            if flags & _INST_OVERFLOW_EX:
                self.ex_cap = max(2 * self.ex_cap, n_ex)
            self.grown += 1
            self._alloc()
            for preds, gts in self.inputs:
                if self.fallback is None:
                    self._enqueue(preds, gts)
        else:
            self.fallback = 'accumulator capacity'
            return None
        out = torch.empty(2 * self.n_seg, dtype=torch.float64, device=self.dev)
        lib = L.lib()
        ws_bytes = lib.sg_inst_curves_workspace_bytes(n_ex, self.n_seg)
        ws = L.workspace(ws_bytes, self.dev)
        L.check(lib.sg_inst_curves(self.ex_key.data_ptr(), self.ex_meta.data_ptr(), n_ex, self.seg_stats.data_ptr(),
                                   self.n_seg, out.data_ptr(), out.data_ptr() + 8 * self.n_seg, self._flags_ptr(),
                                   ws.data_ptr(), ws_bytes, L.stream()), 'sg_inst_curves')
        res = out.cpu().numpy()
        if self.coverage:
            cov = self.cov.cpu().numpy()
            self.cov_result = (cov[:2 * self.n_labels].view(np.float64).reshape(2, self.n_labels).copy(),
                               cov[2 * self.n_labels:].reshape(5, self.n_labels).copy())
        if int(self.meta.cpu()[2]) & _INST_NO_EXAMPLES:
            self.fallback = 'a label with GT and predictions but no example (the reference raises IndexError)'
            return None
        shape = (1, self.n_labels, self.n_thr)
        return res[:self.n_seg].reshape(shape).copy(), res[self.n_seg:].reshape(shape).copy()


class ScanNetEval(object):

    def __init__(self, class_labels, min_npoint=None, iou_type=None, use_label=True, device=None,
                 backend=None, coverage=None):
        self.valid_class_labels = class_labels
        self.valid_class_ids = np.arange(len(class_labels)) + 1
        self.id2label = {int(i): n for i, n in zip(self.valid_class_ids, class_labels)}
        self.label2id = {n: int(i) for i, n in zip(self.valid_class_ids, class_labels)}
        self.ious = np.append(np.arange(0.5, 0.95, 0.05), 0.25)
        self.min_region_sizes = np.array([min_npoint if min_npoint else 100])
        self.distance_threshes = np.array([float('inf')])
        self.distance_confs = np.array([-float('inf')])
        self.iou_type = iou_type
        self.use_label = use_label
        self.eval_class_labels = self.valid_class_labels if use_label else ['class_agnostic']
        self.device = device      # None: GPU when available
        self.backend = backend    # of the streaming form: None / 'host' or 'device'
        self.last_backend = None  # what the last evaluation actually ran on: 'host' or 'device'
        self.last_fallback = None  # why a 'device' evaluation was handed to the host path, or None
        # test hook: initial capacities of the device accumulator, dict(examples=..., gt=...)
        self.device_capacity = None
        # None, or dict(iou_thr, score_thr): mCov / mWCov / mPrec / mRec next to the AP figures
        self.coverage = None
        if coverage:
            given = {} if coverage is True else dict(coverage)
            unknown = sorted(set(given) - {'iou_thr', 'score_thr'})
            if unknown:
                raise ValueError(f'coverage takes iou_thr and score_thr, not {unknown}')
            self.coverage = dict(iou_thr=float(given.get('iou_thr', 0.5)), score_thr=float(given.get('score_thr', 0.0)))
            if np.isnan(self.coverage['iou_thr']) or np.isnan(self.coverage['score_thr']):
                raise ValueError('coverage: iou_thr and score_thr must not be NaN')

    # ------------------------------------------------------------------ association (per scan)
    def _count_matrix(self, starts, lens, run_pred, n_pred, gt_slot, n_slots):
        """counts[p, s] = points of prediction p in GT slot s"""
        import torch
        use_gpu = torch.cuda.is_available() if self.device is None else str(self.device).startswith('cuda')
        if not use_gpu or len(starts) == 0:
            counts = np.zeros((n_pred, n_slots), np.int64)
            for s, n, p in zip(starts.tolist(), lens.tolist(), run_pred.tolist()):
                np.add.at(counts[p], gt_slot[s:s + n], 1)
            return counts
        from .. import _lib as L
        dev = torch.device('cuda' if self.device is None else self.device)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        d_start = torch.from_numpy(starts.astype(np.int32)).to(dev)
        d_off = torch.from_numpy(off).to(dev)
        d_pred = torch.from_numpy(run_pred.astype(np.int32)).to(dev)
        d_slot = torch.from_numpy(gt_slot.astype(np.int32)).to(dev)
        counts = torch.empty((n_pred, n_slots), dtype=torch.int32, device=dev)
        L.check(L.lib().sg_eval_intersections(L.ptr(d_start), L.ptr(d_off), L.ptr(d_pred), len(starts),
                                              int(off[-1]), L.ptr(d_slot), n_pred, n_slots, L.ptr(counts),
                                              L.stream()), 'sg_eval_intersections')
        return counts.cpu().numpy().astype(np.int64)

    def assign_instances_for_scan(self, preds, gts):
        """-> (gt2pred, pred2gt) with the reference's structure: per evaluated label a list of GT
        instance dicts (each with 'matched_pred') and a list of prediction dicts (each with
        'matched_gt'), only the fields the matching reads."""
        gts = np.asarray(gts)
        n_points = gts.shape[0]
        ids, inverse, vert = np.unique(gts, return_inverse=True, return_counts=True)
        lab = ids // 1000
        is_inst = (ids != 0) & np.isin(lab, self.valid_class_ids)
        inst_rows = np.flatnonzero(is_inst)                    # ascending instance id (np.unique order)
        n_gt = len(inst_rows)
        slot_of_id = np.full(len(ids), n_gt, np.int64)         # slot n_gt: not an evaluated instance
        slot_of_id[inst_rows] = np.arange(n_gt)
        gt_slot = slot_of_id[inverse.reshape(-1)]
        # void = points whose CLASS is not evaluated (instance_eval.py:258); points of valid classes
        # with instance id 0 cannot exist (id 0 has class 0)
        gt_label = lab[inst_rows]
        gt_vert = vert[inst_rows]
        gt_ids = ids[inst_rows]

        # predictions that take part (valid label, >= min region size), in list order
        runs_s, runs_l, runs_p, kept = [], [], [], []
        for pred in preds:
            if self.use_label:
                if pred['label_id'] not in self.id2label:
                    continue
            s, n = _runs_of(pred['pred_mask'], n_points)
            num = int(n.sum())
            if num < self.min_region_sizes[0]:
                continue
            runs_s.append(s)
            runs_l.append(n)
            runs_p.append(np.full(len(s), len(kept), np.int64))
            kept.append((pred, num))
        n_pred = len(kept)
        cat = (lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.int64))  # noqa: E731
        counts = self._count_matrix(cat(runs_s), cat(runs_l), cat(runs_p), n_pred, gt_slot, n_gt + 1)

        gt2pred = {label: [] for label in self.eval_class_labels}
        gt_entry = []                                         # per GT slot: its dict
        for g in range(n_gt):
            label = self.id2label[int(gt_label[g])] if self.use_label else self.eval_class_labels[0]
            d = dict(instance_id=int(gt_ids[g]), label_id=int(gt_label[g]), vert_count=int(gt_vert[g]),
                     med_dist=-1, dist_conf=0.0, matched_pred=[])
            gt_entry.append(d)
        if self.use_label:
            for g in range(n_gt):
                gt2pred[self.id2label[int(gt_label[g])]].append(gt_entry[g])
        else:
            # class agnostic: the reference concatenates the per-label lists in label order
            for label in self.valid_class_labels:
                for g in range(n_gt):
                    if self.id2label[int(gt_label[g])] == label:
                        gt2pred[self.eval_class_labels[0]].append(gt_entry[g])
        pred2gt = {label: [] for label in self.eval_class_labels}
        for k, (pred, num) in enumerate(kept):
            label_id = pred['label_id'] if self.use_label else None
            label = self.id2label[label_id] if self.use_label else self.eval_class_labels[0]
            pi = dict(filename='{}_{}'.format(pred['scan_id'], k), pred_id=k, label_id=label_id,
                      vert_count=num, confidence=pred['conf'], void_intersection=int(counts[k, n_gt]))
            matched_gt = []
            for gt in gt2pred[label]:                          # list order, as the reference loops
                g = int(np.searchsorted(gt_ids, gt['instance_id']))
                inter = int(counts[k, g])
                if inter > 0:
                    iou = float(inter) / (gt['vert_count'] + num - inter)
                    gc = {kk: v for kk, v in gt.items() if kk != 'matched_pred'}
                    gc.update(intersection=inter, iou=iou)
                    pc = dict(pi, intersection=inter, iou=iou)
                    matched_gt.append(gc)
                    gt['matched_pred'].append(pc)
            pi['matched_gt'] = matched_gt
            pred2gt[label].append(pi)
        return gt2pred, pred2gt

    # ------------------------------------------------------------------ AP over all scans
    def evaluate_matches(self, matches):
        ious = self.ious
        min_region_size = self.min_region_sizes[0]
        n_lab = len(self.eval_class_labels)
        ap = np.zeros((1, n_lab, len(ious)), float)
        rc = np.zeros((1, n_lab, len(ious)), float)
        for oi, iou_th in enumerate(ious):
            visited = set()                                    # predictions already assigned to a GT
            for li, label_name in enumerate(self.eval_class_labels):
                y_true, y_score = np.empty(0), np.empty(0)
                hard_fn = 0
                has_gt = has_pred = False
                for m in matches:
                    preds = matches[m]['pred'][label_name]
                    gts = [g for g in matches[m]['gt'][label_name]
                           if g['instance_id'] >= 1000 and g['vert_count'] >= min_region_size]
                    has_gt = has_gt or bool(gts)
                    has_pred = has_pred or bool(preds)
                    cur_true = np.ones(len(gts))
                    cur_score = np.ones(len(gts)) * (-float('inf'))
                    cur_match = np.zeros(len(gts), dtype=bool)
                    for gi, gt in enumerate(gts):
                        found = False
                        for pred in gt['matched_pred']:
                            if pred['filename'] in visited:
                                continue
                            if pred['iou'] > iou_th:
                                conf = pred['confidence']
                                if cur_match[gi]:
                                    # a second prediction on a matched GT: the lower score is a false
                                    # positive (and this prediction stays unassigned, as in the reference)
                                    hi, lo = max(cur_score[gi], conf), min(cur_score[gi], conf)
                                    cur_score[gi] = hi
                                    cur_true = np.append(cur_true, 0)
                                    cur_score = np.append(cur_score, lo)
                                    cur_match = np.append(cur_match, True)
                                else:
                                    found = True
                                    cur_match[gi] = True
                                    cur_score[gi] = conf
                                    visited.add(pred['filename'])
                        if not found:
                            hard_fn += 1
                    cur_true = cur_true[cur_match]
                    cur_score = cur_score[cur_match]
                    for pred in preds:                         # unmatched predictions: false positives
                        if any(gt['iou'] > iou_th for gt in pred['matched_gt']):
                            continue
                        ignore = pred['void_intersection']
                        for gt in pred['matched_gt']:
                            if gt['instance_id'] < 1000:
                                ignore += gt['intersection']
                            if gt['vert_count'] < min_region_size:
                                ignore += gt['intersection']
                        if float(ignore) / pred['vert_count'] <= iou_th:
                            cur_true = np.append(cur_true, 0)
                            cur_score = np.append(cur_score, pred['confidence'])
                    y_true = np.append(y_true, cur_true)
                    y_score = np.append(y_score, cur_score)
                if has_gt and has_pred:
                    order = np.argsort(y_score)
                    s_sorted, t_sorted = y_score[order], y_true[order]
                    cum = np.cumsum(t_sorted)
                    _, first = np.unique(s_sorted, return_index=True)
                    n_pr = len(first) + 1
                    n_ex = len(s_sorted)
                    n_true = cum[-1]
                    precision, recall = np.zeros(n_pr), np.zeros(n_pr)
                    cum = np.append(cum, 0)                    # cum[-1] = 0 for the first threshold
                    for i, idx in enumerate(first):
                        below = cum[idx - 1]
                        tp = n_true - below
                        fp = n_ex - idx - tp
                        fn = below + hard_fn
                        precision[i] = float(tp) / (tp + fp)
                        recall[i] = float(tp) / (tp + fn)
                    rc_cur = recall[0]
                    precision[-1], recall[-1] = 1., 0.
                    r = np.append(recall[0], recall)
                    r = np.append(r, 0.)
                    ap_cur = np.dot(precision, np.convolve(r, [-0.5, 0, 0.5], 'valid'))
                elif has_gt:
                    ap_cur = rc_cur = 0.0
                else:
                    ap_cur = rc_cur = float('nan')
                ap[0, li, oi] = ap_cur
                rc[0, li, oi] = rc_cur
        return ap, rc

    # ------------------------------------------------------------------ coverage, precision, recall
    def coverage_of_matches(self, matches):
        """-> (sums float64 [2][n_labels]: cov and wcov summed over the rooms, tallies int64 [5][n_labels]:
        rooms, n_gt, gt_hit, tp, fp) over the scans of `matches` in their order; plain float64 arithmetic in
        the order the module text fixes"""
        iou_thr, score_thr = self.coverage['iou_thr'], self.coverage['score_thr']
        n_lab = len(self.eval_class_labels)
        sums, tallies = np.zeros((2, n_lab), np.float64), np.zeros((5, n_lab), np.int64)
        for m in matches:
            for li, name in enumerate(self.eval_class_labels):
                gts = matches[m]['gt'][name]                   # ascending instance id
                if gts:
                    s, w = np.float64(0.0), np.float64(0.0)
                    vert = hit = 0
                    for gt in gts:
                        ov = 0.0
                        for pred in gt['matched_pred']:
                            if float(pred['confidence']) >= score_thr and pred['iou'] > ov:
                                ov = pred['iou']
                        s = s + np.float64(ov)
                        w = w + np.float64(ov) * np.float64(gt['vert_count'])
                        vert += gt['vert_count']
                        hit += 1 if ov >= iou_thr else 0
                    tallies[0, li] += 1
                    tallies[1, li] += len(gts)
                    tallies[2, li] += hit
                    sums[0, li] = sums[0, li] + s / np.float64(len(gts))
                    sums[1, li] = sums[1, li] + w / np.float64(vert)
                for pred in matches[m]['pred'][name]:
                    if not float(pred['confidence']) >= score_thr:
                        continue
                    ov = max((gt['iou'] for gt in pred['matched_gt']), default=0.0)
                    tallies[3 if ov >= iou_thr else 4, li] += 1
        return sums, tallies

    def add_coverage_averages(self, avgs, sums, tallies):
        rooms, n_gt, hit, tp, fp = (tallies[i] for i in range(5))
        with np.errstate(divide='ignore', invalid='ignore'):
            cols = dict(cov=sums[0] / rooms, wcov=sums[1] / rooms, prec=tp / (tp + fp), rec=hit / n_gt)
        for key, v in cols.items():
            with warnings.catch_warnings():                    # every label NaN: NaN, quietly
                warnings.simplefilter('ignore', RuntimeWarning)
                avgs['all_' + key] = np.nanmean(v)
            for li, name in enumerate(self.eval_class_labels):
                avgs['classes'][name][key] = v[li]
        avgs['coverage_counts'] = {k: tallies[i].astype(np.int64) for i, k in enumerate(_COV_TALLIES)}
        return avgs

    def compute_averages(self, aps, rcs):
        o50 = np.where(np.isclose(self.ious, 0.5))
        o25 = np.where(np.isclose(self.ious, 0.25))
        rest = np.where(np.logical_not(np.isclose(self.ious, 0.25)))
        avg = {'all_ap': np.nanmean(aps[0, :, rest]), 'all_ap_50%': np.nanmean(aps[0, :, o50]),
               'all_ap_25%': np.nanmean(aps[0, :, o25]), 'all_rc': np.nanmean(rcs[0, :, rest]),
               'all_rc_50%': np.nanmean(rcs[0, :, o50]), 'all_rc_25%': np.nanmean(rcs[0, :, o25]),
               'classes': {}}
        for li, name in enumerate(self.eval_class_labels):
            avg['classes'][name] = {
                'ap': np.average(aps[0, li, rest]), 'ap50%': np.average(aps[0, li, o50]),
                'ap25%': np.average(aps[0, li, o25]), 'rc': np.average(rcs[0, li, rest]),
                'rc50%': np.average(rcs[0, li, o50]), 'rc25%': np.average(rcs[0, li, o25])}
        return avg

    def evaluate(self, pred_list, gt_list, verbose=True, backend=None):
        """pred_list: per scan a list of dict(scan_id, label_id, conf, pred_mask (RLE dict or array));
        gt_list: per scan an array of class_id * 1000 + instance_id per point (0 = unannotated).
        backend: None / 'host' (the path above) or 'device' (the whole evaluation in HIP)."""
        if backend not in (None, 'host', 'device'):
            raise ValueError(f"backend must be None, 'host' or 'device', not {backend!r}")
        if backend == 'device':
            self.reset(backend='device')
            for preds, gts in zip(pred_list, gt_list):
                self.update(preds, gts)
            return self.compute(verbose=verbose)
        self.last_backend, self.last_fallback = 'host', None
        matches = {}
        for i, (preds, gts) in enumerate(zip(pred_list, gt_list)):
            gt2pred, pred2gt = self.assign_instances_for_scan(preds, gts)
            matches[f'gt_{i}'] = {'gt': gt2pred, 'pred': pred2gt}
        avgs = self.compute_averages(*self.evaluate_matches(matches))
        if self.coverage:
            self.add_coverage_averages(avgs, *self.coverage_of_matches(matches))
        if verbose:
            self.print_results(avgs)
        return avgs

    # ------------------------------------------------------------------ streaming form
    def reset(self, backend=None):
        """Starts an evaluation that is fed one scan at a time: reset(), update(preds, gts) per scan,
        compute().  backend: as for evaluate (default: the constructor's)."""
        backend = self.backend if backend is None else backend
        if backend not in (None, 'host', 'device'):
            raise ValueError(f"backend must be None, 'host' or 'device', not {backend!r}")
        self._stream_backend = 'device' if backend == 'device' else 'host'
        self._matches = {}
        self._dev = None
        if self._stream_backend == 'device':
            self._dev = _DeviceAccumulator(self)

    def update(self, preds, gts):
        """One scan.  Host backend: its matches are stored.  Device backend: the scan's inputs are copied
        through pinned staging and its kernels are enqueued on the current stream -- nothing is read back."""
        if getattr(self, '_stream_backend', None) is None:
            self.reset()
        if self._dev is not None:
            self._dev.update(preds, gts)
        else:
            gt2pred, pred2gt = self.assign_instances_for_scan(preds, gts)
            self._matches[f'gt_{len(self._matches)}'] = {'gt': gt2pred, 'pred': pred2gt}

    def compute(self, verbose=False):
        """-> the averages over the scans given to update() since reset()."""
        if getattr(self, '_stream_backend', None) is None:
            self.reset()
        if self._dev is not None:
            res = self._dev.compute()
            if res is None:                                    # handed to the host path, with the reason
                self.last_backend, self.last_fallback = 'host', self._dev.fallback
                matches = {}
                for i, (preds, gts) in enumerate(self._dev.inputs):
                    gt2pred, pred2gt = self.assign_instances_for_scan(preds, _host_gts(gts))
                    matches[f'gt_{i}'] = {'gt': gt2pred, 'pred': pred2gt}
                res = self.evaluate_matches(matches)
                cov = self.coverage_of_matches(matches) if self.coverage else None
            else:
                self.last_backend, self.last_fallback = 'device', None
                cov = self._dev.cov_result if self.coverage else None
        else:
            self.last_backend, self.last_fallback = 'host', None
            res = self.evaluate_matches(self._matches)
            cov = self.coverage_of_matches(self._matches) if self.coverage else None
        avgs = self.compute_averages(*res)
        if cov is not None:
            self.add_coverage_averages(avgs, *cov)
        if verbose:
            self.print_results(avgs)
        return avgs

    def print_results(self, avgs):
        width = 64
        cols = ('AP', 'AP_50%', 'AP_25%', 'AR', 'RC_50%', 'RC_25%')
        print()
        print('#' * width)
        print('{:<15}'.format('what') + ':' + ''.join('{:>8}'.format(c) for c in cols))
        print('#' * width)
        keys = ('ap', 'ap50%', 'ap25%', 'rc', 'rc50%', 'rc25%')
        for name in self.eval_class_labels:
            c = avgs['classes'][name]
            print('{:<15}'.format(name) + ':' + ''.join('{:>8.3f}'.format(c[k]) for k in keys))
        print('-' * width)
        alls = ('all_ap', 'all_ap_50%', 'all_ap_25%', 'all_rc', 'all_rc_50%', 'all_rc_25%')
        print('{:<15}'.format('average') + ':' + ''.join('{:>8.3f}'.format(avgs[k]) for k in alls))
        print('#' * width)
        print()
        if 'all_cov' in avgs:
            cols, keys = ('mCov', 'mWCov', 'mPrec', 'mRec'), ('cov', 'wcov', 'prec', 'rec')
            print('#' * width)
            print('{:<15}'.format('what') + ':' + ''.join('{:>8}'.format(c) for c in cols))
            print('#' * width)
            for name in self.eval_class_labels:
                c = avgs['classes'][name]
                print('{:<15}'.format(name) + ':' + ''.join('{:>8.3f}'.format(c[k]) for k in keys))
            print('-' * width)
            print('{:<15}'.format('average') + ':' + ''.join('{:>8.3f}'.format(avgs['all_' + k]) for k in keys))
            print('#' * width)
            print()

    def write_result_file(self, avgs, filename):
        with open(filename, 'w') as f:
            f.write(','.join(['class', 'class id', 'ap', 'ap50', 'ap25']) + '\n')
            for name in self.eval_class_labels:
                c = avgs['classes'][name]
                f.write(','.join(str(x) for x in [name, c['ap'], c['ap50%'], c['ap25%']]) + '\n')
