"""Mirror of ``softgroup.ops`` (reference: softgroup/ops/__init__.py star-imports functions.py)."""
from .functions import *  # noqa: F401,F403
from .functions import (ball_query, ballquery_batch_p, bfs_cluster, bfs_cluster_segments,  # noqa: F401
                        get_mask_iou_on_cluster, get_mask_iou_on_pred, get_mask_label,
                        global_avg_pool, octree_ball_query, sec_max, sec_mean, sec_min,
                        voxelization, voxelization_idx)
from .losses import assign_proposals, instance_losses, point_wise_loss  # noqa: F401
from .nms import mask_bits_from_runs, mask_nms, mask_nms_numpy  # noqa: F401
from .resample import (grid_downsample, mask_bits_gather, mask_runs_from_bits,  # noqa: F401
                       nearest_index)
from .geometry import (grow_segments, grow_segments_numpy, knn, knn_numpy, point_normals,  # noqa: F401
                       point_normals_numpy)
from .boxes import (box_iou, box_iou_numpy, box_nms, box_nms_numpy, boxes8,  # noqa: F401
                    obb_iou_pair)
from .split import mask_components, mask_components_numpy  # noqa: F401
from .superpoint import (SuperpointIndex, mask_snap, mask_snap_numpy, superpoint_index,  # noqa: F401
                         superpoint_index_numpy, superpoint_vote, superpoint_vote_numpy)
from .stitch import (mask_cross_links, stitch_components, stitch_union, tile_assign,  # noqa: F401
                     tile_shared)
from .ensemble import (label_vote, label_vote_numpy, mask_group_links, mask_group_links_numpy,  # noqa: F401
                       mask_vote, mask_vote_numpy)
