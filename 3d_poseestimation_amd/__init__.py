"""MI355X-native 2D->3D pose-lifting train path (the hot path of RHnejad/3D_PoseEstimation).

Import as `importlib.import_module("3d_poseestimation_amd")` or through the `poselift`
alias module at the repository root.
"""
from ._lib import PoseliftError, lib  # noqa: F401
from .model import Linear, LinearModel, weight_init  # noqa: F401
from .optim import FlatAdamW, FlatOptimizer  # noqa: F401
from .arena import FlatAdam, ModuleArena  # noqa: F401
from .train import (crop_poses, cycle_step, epoch_mpjpe_mm, eval_step, flip_average, flip_frames_nhwc, flip_pose, loss_MPJPE, mse_loss,  # noqa: F401
                    predict_flip_tta, train_step, uncrop_poses, GraphedTrainStep, GraphedModuleStep)
from .heads import (gaussian_heatmap, heatmap_law, soft_argmax_2d, soft_argmax_2d_hm, soft_argmax_3d,  # noqa: F401
                    soft_argmax_3d_hm, soft_argmax_3d_nhwc, soft_argmax_3d_nhwc_hm)
from .losses import TriangleLoss, heatmap_mse, l1_loss, l1_terms  # noqa: F401
from .criterion import H36M_SKELETON, PoseCriterion, Skeleton, bone_lengths, normalize_row_weights  # noqa: F401
from .metrics import AUC_THRESHOLDS, PoseMetrics, pose_errors, procrustes_align  # noqa: F401
from .backbone import Model_2D, Model_3D, ResNet  # noqa: F401
from .data import (FrameFeeder, PersonCrop, PoseAugment, PoseFeeder, augment_frames, augment_poses, crop_boxes, gather_row_weights,  # noqa: F401
                   epoch_indices)
from .pose_table import H36M_17_OF_32, PoseStats, PoseTransform, pose_stats, prepare_poses  # noqa: F401
from .sequence import (SequenceLifter, TemporalFilter, coco_to_h36m, filter_tracks, load_keypoints_json, prepare_tracks,  # noqa: F401
                       velocity_errors)
from .camera import CameraTable, fit_translation, project_poses, reprojection_errors, reprojection_loss  # noqa: F401
from .vit import MyViT  # noqa: F401
from .range_guard import PoseliftRangeError  # noqa: F401
from . import arena, backbone, camera, conv, data, dp, gradclip, layout, metrics, pose_table, range_guard, sequence, synth, vit  # noqa: F401
