"""semantic_slam_mapping_amd -- MI355X (gfx950) per-frame semantic-mapping front end.

The product is the C-ABI library ``libssm_hip.so`` (include/ssm_hip.h, sources in csrc/) and the C++ host classes in
include/ssm/.  This package is the Python mirror of that boundary used by tests and bench.py: thin ctypes calls,
numpy only for host buffers.  It has no CPU fallback -- a missing library or a missing GPU raises.
"""
from .api import Context, Tracker, Vocabulary, Looper, vocab_kmajority, motion_fuse_host, motion_fuse_tile, sor_filter_host, sor_chunk, pnp_lds_edge_capacity,carve_host, render_host, render_compare_host, label_colours, align_host, align_params, grid_host, grid_params, grid_frame_from_up, grid_colours, GRID_CELL_DTYPE, objects_host, objects_cells_host, objects_params, OBJECT_DTYPE, clearance_cells_host, clearance_params, route_cells_host, route_path_host, route_params, relabel_host, relabel_params, relabel_labels_host, UVDisparity, PoseGraphOptimizer, GlibcRand, SsmError, default_config, live_allocations, live_handles, KEYPOINT_DTYPE, DMATCH_DTYPE, POINT_DTYPE, VOXEL_DTYPE, PMATCH_DTYPE, UVD_INFO_DTYPE, PGO_REPORT_DTYPE, MOTION_FUSE_INFO_DTYPE  # noqa: F401
from ._lib import LIB_PATH, SYMBOLS, load  # noqa: F401
