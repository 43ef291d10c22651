from .instance_eval import ScanNetEval
from .panoptic_eval import PanopticEval
from .point_wise_eval import evaluate_offset_mae, evaluate_semantic_acc, evaluate_semantic_miou

__all__ = ['ScanNetEval', 'PanopticEval', 'evaluate_semantic_acc', 'evaluate_semantic_miou', 'evaluate_offset_mae']
