from .cast import cuda_cast, force_fp32, to_host, to_host_begin, to_host_end  # noqa: F401
from .rle import (rle_decode, rle_encode, rle_encode_many, rle_encode_runs,  # noqa: F401
                  rle_text_to_dicts)  # noqa: F401
from .results import (load_pred_instances, read_int_lines, read_mask, save_gt_instances,  # noqa: F401
                      save_npy, save_panoptic, save_pred_instances, save_results)  # noqa: F401
from .visualize import (colors_from_result, get_coords_color, save_visualizations,  # noqa: F401
                        write_ply)  # noqa: F401
from .nms import nms_instances  # noqa: F401
from .split import split_instances  # noqa: F401
from .propagate import propagate_result  # noqa: F401
from .stitch import stitch_results  # noqa: F401
from .ensemble import ensemble_results  # noqa: F401
from .superpoint import load_scannet_segs, refine_result, snap_instances  # noqa: F401
from .geometry import make_superpoints  # noqa: F401
from .objects import (ObjectTable, box_corners, describe_instances, describe_result,  # noqa: F401
                      load_objects, save_objects)  # noqa: F401
from .boxes import nms_boxes, nms_objects, take_rows  # noqa: F401
from .cloud_io import read_cloud, read_ply, read_table  # noqa: F401
from .render import (fit_view, look_at, montage, read_png, render_cloud, render_result,  # noqa: F401
                     save_renders, turntable, write_png)  # noqa: F401
from ..optim import build_optimizer, clip_grad_norm_  # noqa: F401,E402
