"""The loss block of ``forward_train`` (reference softgroup/model/softgroup.py:152-255) on the fused
kernels of csrc/losses.hip: one forward and one backward launch per group of losses instead of the
~40 small torch kernels (and their autograd) of the expression form.

Three public functions, each an autograd node around the C entries:

  point_wise_loss   sg_pointwise_loss_fwd / _bwd     semantic cross entropy + offset L1
  assign_proposals  sg_assign_proposals              proposal -> class label (no gradient)
  instance_losses   sg_mask_loss_* , sg_proposal_loss_*   cls / mask / iou_score loss, num_pos, num_neg

Inputs are cast to float32 for the kernels and gradients come back in the input's dtype (bf16
autocast).  CPU tensors, and class counts outside the kernels' 64-column range, take the torch
expressions of model/softgroup.py -- the same values, so the functions can be compared with
F.cross_entropy / F.binary_cross_entropy on the CPU.  Nothing here reads back from the device.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib as L

MAX_CLASSES = 64          # kLossMaxC of csrc/losses.hip


def _f32(t):
    return t.detach().float().contiguous()


def _i64(t):
    return t.detach().long().contiguous()


def _scalar(g):
    """upstream gradient of a scalar loss as a float32 device scalar; None stays None (= zero)"""
    return None if g is None else g.detach().float().contiguous()


def _reduce_ws(dev):
    return L.workspace(L.lib().sg_loss_reduce_workspace_bytes(), dev)


# ---------------------------------------------------------------------------------------------
# point-wise losses
# ---------------------------------------------------------------------------------------------
class _PointWiseLoss(Function):

    @staticmethod
    def forward(ctx, semantic_scores, pt_offsets, semantic_labels, instance_labels, pt_offset_labels,
                weight, ignore_label):
        n, c = semantic_scores.shape
        s, o, ol = _f32(semantic_scores), _f32(pt_offsets), _f32(pt_offset_labels)
        sl, il = _i64(semantic_labels), _i64(instance_labels)
        w = None if weight is None else _f32(weight)
        out = torch.empty(6, dtype=torch.float32, device=s.device)
        ws = _reduce_ws(s.device)
        L.check(L.lib().sg_pointwise_loss_fwd(
            L.ptr(s), L.ptr(sl), L.ptr(w), int(ignore_label), L.ptr(o), L.ptr(ol), L.ptr(il), n, c,
            L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), 'sg_pointwise_loss_fwd')
        ctx.save_for_backward(s, o, ol, sl, il, out, *(() if w is None else (w, )))
        ctx.ignore_label = int(ignore_label)
        ctx.dtypes = (semantic_scores.dtype, pt_offsets.dtype)
        ctx.set_materialize_grads(False)
        return out[4], out[5]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_sem, g_off):
        s, o, ol, sl, il, out, *w = ctx.saved_tensors
        w = w[0] if w else None
        n, c = s.shape
        d_s = torch.empty_like(s) if ctx.needs_input_grad[0] else None
        d_o = torch.empty_like(o) if ctx.needs_input_grad[1] else None
        gs, go = _scalar(g_sem), _scalar(g_off)
        L.check(L.lib().sg_pointwise_loss_bwd(
            L.ptr(s), L.ptr(sl), L.ptr(w), ctx.ignore_label, L.ptr(o), L.ptr(ol), L.ptr(il), n, c,
            L.ptr(out), L.ptr(gs), L.ptr(go), L.ptr(d_s), L.ptr(d_o), L.stream()), 'sg_pointwise_loss_bwd')
        if d_s is not None:
            d_s = d_s.to(ctx.dtypes[0])
        if d_o is not None:
            d_o = d_o.to(ctx.dtypes[1])
        return d_s, d_o, None, None, None, None, None


def _point_wise_loss_torch(semantic_scores, pt_offsets, semantic_labels, instance_labels, pt_offset_labels,
                           weight, ignore_label):
    from ..model.softgroup import _cross_entropy
    semantic_loss = _cross_entropy(semantic_scores, semantic_labels, weight, ignore_label)
    pos = (instance_labels != ignore_label)
    n_pos = pos.sum(dtype=torch.int32)
    diff = (pt_offsets - pt_offset_labels).abs()
    diff = torch.where(pos.unsqueeze(1), diff, torch.zeros((), dtype=diff.dtype, device=diff.device))
    return semantic_loss, diff.sum() / n_pos.clamp(min=1)


def point_wise_loss(semantic_scores, pt_offsets, semantic_labels, instance_labels, pt_offset_labels,
                    weight=None, ignore_label=-100):
    """-> (semantic_loss, offset_loss) of softgroup.py:152-170: F.cross_entropy(weight=,
    ignore_index=) over all points, L1 offset loss over the points of instances (0 without one)."""
    if not (semantic_scores.is_cuda and 1 <= semantic_scores.shape[1] <= MAX_CLASSES):
        return _point_wise_loss_torch(semantic_scores, pt_offsets, semantic_labels, instance_labels,
                                      pt_offset_labels, weight, ignore_label)
    return _PointWiseLoss.apply(semantic_scores, pt_offsets, semantic_labels, instance_labels,
                                pt_offset_labels, weight, ignore_label)


# ---------------------------------------------------------------------------------------------
# proposal assignment
# ---------------------------------------------------------------------------------------------
class _AssignProposals(Function):

    @staticmethod
    def forward(ctx, ious_on_cluster, instance_cls, ignore_label, pos_iou_thr, match_low_quality, min_pos_thr,
                background_label):
        n_prop, n_gt = ious_on_cluster.shape
        ious, cls = _f32(ious_on_cluster), _i64(instance_cls)
        labels = torch.empty(n_prop, dtype=torch.int64, device=ious.device)
        lib = L.lib()
        ws = L.workspace(lib.sg_assign_proposals_workspace_bytes(n_prop) if match_low_quality else 0, ious.device)
        L.check(lib.sg_assign_proposals(
            L.ptr(ious), L.ptr(cls), int(ignore_label), float(pos_iou_thr), int(bool(match_low_quality)),
            float(min_pos_thr), int(background_label), n_prop, n_gt, L.ptr(labels), L.ptr(ws), ws.numel(),
            L.stream()), 'sg_assign_proposals')
        ctx.mark_non_differentiable(labels)
        return labels

    @staticmethod
    def backward(ctx, a=None):
        return None, None, None, None, None, None, None


def assign_proposals(ious_on_cluster, instance_cls, ignore_label=-100, pos_iou_thr=0.5, match_low_quality=False,
                     min_pos_thr=0, background_label=18):
    """-> labels int64 [n_proposal] of softgroup.py:194-222 (``_assign_proposals`` of model/softgroup.py)."""
    if not ious_on_cluster.is_cuda or ious_on_cluster.shape[1] < 1:
        from ..model.softgroup import _assign_proposals
        return _assign_proposals(ious_on_cluster, instance_cls, instance_cls != ignore_label, pos_iou_thr,
                                 match_low_quality, min_pos_thr, background_label)
    return _AssignProposals.apply(ious_on_cluster, instance_cls, ignore_label, pos_iou_thr, match_low_quality,
                                  min_pos_thr, background_label)


# ---------------------------------------------------------------------------------------------
# proposal-level and mask losses
# ---------------------------------------------------------------------------------------------
class _MaskLoss(Function):
    """-> (mask_loss, mask_sig); mask_sig carries no gradient (the reference detaches it, :241-242)"""

    @staticmethod
    def forward(ctx, mask_scores, instance_batch_idxs, labels, mask_label):
        m, k1 = mask_scores.shape
        s, ml = _f32(mask_scores), _f32(mask_label)
        bi, lab = instance_batch_idxs.detach().int().contiguous(), _i64(labels)
        sig = torch.empty(m, dtype=torch.float32, device=s.device)
        out = torch.empty(6, dtype=torch.float32, device=s.device)
        ws = _reduce_ws(s.device)
        L.check(L.lib().sg_mask_loss_fwd(
            L.ptr(s), L.ptr(bi), L.ptr(lab), L.ptr(ml), m, lab.numel(), k1, L.ptr(sig), L.ptr(out), L.ptr(ws),
            ws.numel(), L.stream()), 'sg_mask_loss_fwd')
        ctx.save_for_backward(s, bi, lab, ml, out)
        ctx.dtype = mask_scores.dtype
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(sig)
        return out[4], sig

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_sig=None):
        s, bi, lab, ml, out = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        m, k1 = s.shape
        d = torch.empty_like(s)
        g = _scalar(g_loss)
        L.check(L.lib().sg_mask_loss_bwd(
            L.ptr(s), L.ptr(bi), L.ptr(lab), L.ptr(ml), L.ptr(out), L.ptr(g), m, lab.numel(), k1, L.ptr(d),
            L.stream()), 'sg_mask_loss_bwd')
        return d.to(ctx.dtype), None, None, None


class _ProposalLoss(Function):
    """-> (cls_loss, iou_score_loss, num_pos, num_neg)"""

    @staticmethod
    def forward(ctx, cls_scores, iou_scores, labels, ious_on_pred, instance_cls, ignore_label):
        n_prop, k1 = cls_scores.shape
        cs, io, lab = _f32(cls_scores), _f32(iou_scores), _i64(labels)
        ious, cls = _f32(ious_on_pred), _i64(instance_cls)
        gt_iou = torch.empty(n_prop, dtype=torch.float32, device=cs.device)
        out = torch.empty(6, dtype=torch.float32, device=cs.device)
        ws = _reduce_ws(cs.device)
        L.check(L.lib().sg_proposal_loss_fwd(
            L.ptr(cs), L.ptr(io), L.ptr(lab), L.ptr(ious), L.ptr(cls), int(ignore_label), n_prop, cls.numel(), k1,
            L.ptr(gt_iou), L.ptr(out), L.ptr(ws), ws.numel(), L.stream()), 'sg_proposal_loss_fwd')
        ctx.save_for_backward(cs, io, lab, gt_iou, out)
        ctx.dtypes = (cls_scores.dtype, iou_scores.dtype)
        ctx.set_materialize_grads(False)
        num_pos, num_neg = out[2], out[3]
        ctx.mark_non_differentiable(num_pos, num_neg)
        return out[4], out[5], num_pos, num_neg

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_iou, g_pos=None, g_neg=None):
        cs, io, lab, gt_iou, out = ctx.saved_tensors
        n_prop, k1 = cs.shape
        d_c = torch.empty_like(cs) if ctx.needs_input_grad[0] else None
        d_i = torch.empty_like(io) if ctx.needs_input_grad[1] else None
        gc, gi = _scalar(g_cls), _scalar(g_iou)
        L.check(L.lib().sg_proposal_loss_bwd(
            L.ptr(cs), L.ptr(io), L.ptr(lab), L.ptr(gt_iou), L.ptr(out), L.ptr(gc), L.ptr(gi), n_prop, k1,
            L.ptr(d_c), L.ptr(d_i), L.stream()), 'sg_proposal_loss_bwd')
        if d_c is not None:
            d_c = d_c.to(ctx.dtypes[0])
        if d_i is not None:
            d_i = d_i.to(ctx.dtypes[1])
        return d_c, d_i, None, None, None, None


def _instance_losses_torch(cls_scores, mask_scores, iou_scores, labels, instance_batch_idxs, mask_label,
                           instance_cls, iou_on_pred, ignore_label, instance_classes):
    """the expressions of SoftGroup.instance_loss (model/softgroup.py), reference softgroup.py:223-255"""
    dev = cls_scores.device
    losses = dict(cls_loss=F.cross_entropy(cls_scores, labels))
    per_point_cls = labels[instance_batch_idxs.long()]
    rows = torch.arange(per_point_cls.size(0), device=dev)
    mask_sig = mask_scores.sigmoid()[rows, per_point_cls]
    weight = (mask_label != -1).to(mask_sig.dtype)
    mask_label = torch.where(mask_label == -1., mask_label.new_full((), 0.5), mask_label).to(mask_sig.dtype)
    mask_loss = F.binary_cross_entropy(mask_sig, mask_label, weight=weight, reduction='sum')
    losses['mask_loss'] = mask_loss / (weight.sum() + 1)
    ious = iou_on_pred(mask_sig.detach().contiguous())
    fg = instance_cls != ignore_label
    gt_ious, _ = torch.where(fg.unsqueeze(0), ious, ious.new_full((), -1.0)).max(1)
    rows = torch.arange(labels.size(0), device=dev)
    w = (labels < instance_classes).to(iou_scores.dtype)
    iou_loss = F.mse_loss(iou_scores[rows, labels], gt_ious.to(iou_scores.dtype), reduction='none')
    losses['iou_score_loss'] = (iou_loss * w).sum() / (w.sum() + 1)
    losses['num_pos'] = (labels < instance_classes).sum().float()
    losses['num_neg'] = (labels >= instance_classes).sum().float()
    return losses


def instance_losses(cls_scores, mask_scores, iou_scores, labels, instance_batch_idxs, mask_label, instance_cls,
                    iou_on_pred, ignore_label=-100, instance_classes=18):
    """-> dict(cls_loss, mask_loss, iou_score_loss, num_pos, num_neg) of softgroup.py:223-255 for the
    proposals' class ``labels`` (``assign_proposals``) and the points' ``mask_label`` (``get_mask_label``).
    ``iou_on_pred(mask_sig)`` -> [n_proposal, n_gt] is called between the two kernels with the detached
    sigmoid of every point's assigned-class mask score (``get_mask_iou_on_pred`` in the model)."""
    k1 = cls_scores.shape[1]
    if not (cls_scores.is_cuda and 2 <= k1 <= MAX_CLASSES and k1 == instance_classes + 1
            and mask_scores.shape[1] == k1 and iou_scores.shape[1] == k1 and instance_cls.numel() >= 1):
        return _instance_losses_torch(cls_scores, mask_scores, iou_scores, labels, instance_batch_idxs,
                                      mask_label, instance_cls, iou_on_pred, ignore_label, instance_classes)
    mask_loss, mask_sig = _MaskLoss.apply(mask_scores, instance_batch_idxs, labels, mask_label)
    ious = iou_on_pred(mask_sig)
    cls_loss, iou_loss, num_pos, num_neg = _ProposalLoss.apply(cls_scores, iou_scores, labels, ious, instance_cls,
                                                               ignore_label)
    return dict(cls_loss=cls_loss, mask_loss=mask_loss, iou_score_loss=iou_loss, num_pos=num_pos, num_neg=num_neg)
