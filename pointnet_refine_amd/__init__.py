"""MI355X-native LineRefineNet hot path (shared-MLP context encoder, pooling,
context_proj, line point-MLP) behind the reference's nn.Module surface.

    from pointnet_refine_amd.model import LineRefineNet   # drop-in for src.model
"""
from .model import (DetrTransformerDecoderLayer, LineRefineNet, MultiScalePointNetEncoder,  # noqa: F401
                    PositionalEncoding)
from .metrics import (calibrate_alignment, calibrate_alignments, evaluate_scene, evaluate_scenes,  # noqa: F401
                      line_metrics, shift_sweep, shift_sweep_ragged)
from .support import map_support, marking_attributes, node_support  # noqa: F401
from .ground import ground_heights, lift_lines, line_stations  # noqa: F401
from .align import align_lines, paint_scores, pick_shift, shift_grid  # noqa: F401
from .trace import paint_peaks, refine_cloud, trace_lines  # noqa: F401
from .paintfloor import otsu_floors, paint_floor, surface_ground, surface_histograms  # noqa: F401

__all__ = ["LineRefineNet", "MultiScalePointNetEncoder", "PositionalEncoding",
           "DetrTransformerDecoderLayer",
           "line_metrics", "shift_sweep", "calibrate_alignment", "evaluate_scene",
           "shift_sweep_ragged", "calibrate_alignments", "evaluate_scenes",
           "node_support", "map_support", "marking_attributes",
           "ground_heights", "line_stations", "lift_lines",
           "paint_scores", "align_lines", "pick_shift", "shift_grid",
           "paint_peaks", "trace_lines", "refine_cloud",
           "paint_floor", "surface_ground", "surface_histograms", "otsu_floors"]
