from .det_eval import (eval_det, eval_det_cls, eval_sphere, evaluate_box_ap, get_iou,  # noqa: F401
                       get_iou_bev, get_iou_obb, oriented_instance_boxes, voc_ap)
from .instance_eval import ScanNetEval
from .panoptic_eval import PanopticEval
from .point_wise_eval import evaluate_offset_mae, evaluate_semantic_acc, evaluate_semantic_miou

# (the box-AP functions above are importable from here; __all__ keeps listing the reference's evaluation
# package, which tools/eval_det.py's functions are not part of)
__all__ = ['ScanNetEval', 'PanopticEval', 'evaluate_semantic_acc', 'evaluate_semantic_miou', 'evaluate_offset_mae']
