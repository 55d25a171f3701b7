"""ctypes binding of libdspmap_hip.so (include/dspmap.h).

Host-side mirror of the reference's `class DSPMap` surface
(include/dsp_dynamic.h:142-446,1550-1584 of g-ch/DSP-map): same method names,
argument meaning and return contract, forwarding to the C ABI.  There is no
CPU path in here: if the shared library is missing, or no HIP device is
usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdspmap_hip.so")

MAX_PRED = 16
OK, REJECTED = 1, 0

P_POSITION_STDDEV, P_VELOCITY_STDDEV, P_OBSERVATION_STDDEV, P_NEWBORN_WEIGHT, P_NEWBORN_NUMBER, \
    P_VOXEL_FILTER_RES, P_KAPPA, P_DETECTION, P_VELOCITY_ESTIMATOR, P_REGENERATE_TABLES, P_USE_GRAPH, P_OCCLUSION_MARGIN, \
    P_PAIR_CULL_SIGMAS, P_UPDATE_TIME, P_UPDATE_COUNTER, P_PLACE_SPLIT_TILES, P_FAST_DIVISION, P_SPARSE_SWEEP, P_ROLLOUT_INLINE, \
    P_RESAMPLE_WG_TILES, P_SWEEP_ALTERNATE, P_STATIC_TILE_SKIP, P_HOST_CLOUD_DIRECT, _P_REMOVED_24, P_ESTIMATOR_QUEUE, P_FRAME_BRANCHES, P_TILING, P_SIDE_PLACEMENT, P_RESAMPLE_SPLIT, P_TILE_BITMAPS, P_VIEW_CHUNKS, P_FRONTIER_MERGE, P_PAIR_PREPARE = range(1, 34)


class Config(C.Structure):
    _fields_ = [
        ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
        ("voxel_resolution", C.c_float),
        ("angle_resolution", C.c_int),
        ("max_particle_num_voxel", C.c_int),
        ("half_fov_h", C.c_int), ("half_fov_v", C.c_int),
        ("prediction_times", C.c_int),
        ("prediction_future_time", C.c_float * MAX_PRED),
        ("z_lo", C.c_int), ("z_hi", C.c_int),
        ("device", C.c_int),
        ("gaussian_table_size", C.c_int),
        ("seed", C.c_uint),
        ("pyramid_neighbor_n", C.c_int), ("safe_particle_factor", C.c_int), ("static_model", C.c_int),
    ]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "n_points_in", "n_valid", "n_obs", "n_live_in", "n_moved", "n_out_of_map", "n_voxel_full",
        "n_pyramid_full", "n_fov", "n_born", "n_born_dropped", "n_live_out", "n_exported_up",
        "n_exported_down", "n_reslotted", "n_overflow_inexact")] + [("newborn_weight", C.c_float), ("update_ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Camera(C.Structure):
    """dspmap_camera: the depth image's layout, the pinhole intrinsics and which pixels are used (include/dspmap.h)"""
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int),
        ("row_stride_bytes", C.c_int),
        ("format", C.c_int),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("depth_scale", C.c_float),
        ("min_depth", C.c_float), ("max_depth", C.c_float),
        ("pixel_step", C.c_int),
    ]


DEPTH_U16, DEPTH_F32 = 0, 1   # DSPMAP_DEPTH_*


def make_camera(width, height, fx, fy, cx, cy, depth_scale=0.001, min_depth=0.0, max_depth=20.0, fmt=DEPTH_U16, row_stride_bytes=0,
                pixel_step=1):
    c = Camera()
    c.width, c.height, c.row_stride_bytes, c.format = width, height, row_stride_bytes, fmt
    c.fx, c.fy, c.cx, c.cy = fx, fy, cx, cy
    c.depth_scale, c.min_depth, c.max_depth, c.pixel_step = depth_scale, min_depth, max_depth, pixel_step
    return c


VPOINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"),
                         ("nx", "f4"), ("ny", "f4"), ("nz", "f4"), ("intensity", "f4")])
# dspmap_risk: one per trajectory (dspmap_trajectory_risk)
RISK_DTYPE = np.dtype([("sum", "f4"), ("max", "f4"), ("first_over", "i4"), ("n_outside", "i4")])
QUERY_WORLD = 1   # DSPMAP_QUERY_WORLD
DIST_OUTSIDE_OCCUPIED = 1   # DSPMAP_DIST_OUTSIDE_OCCUPIED
# dspmap_nearest (dspmap_query_nearest) and the DSPMAP_NEAREST_* flags
NEAREST_DTYPE = np.dtype([("dist", "f4"), ("voxel", "i4"), ("offset", "f4", (3,)), ("velocity", "f4", (3,))])
NEAREST_SIGNED, NEAREST_FROM_CAST_GRID = 1, 2
# dspmap_segment / dspmap_cast_hit (dspmap_cast_segments) and the DSPMAP_CAST_* statuses
SEGMENT_DTYPE = np.dtype([("ax", "f4"), ("ay", "f4"), ("az", "f4"), ("ta", "f4"), ("bx", "f4"), ("by", "f4"), ("bz", "f4"), ("tb", "f4")])
HIT_DTYPE = np.dtype([("s", "f4"), ("voxel", "i4"), ("layer", "i4"), ("status", "i4")])
CAST_FREE, CAST_HIT, CAST_LEFT_MAP, CAST_START_OUTSIDE, CAST_INVALID = range(5)
CAST_MAX_INFLATE = 8   # DSPMAP_CAST_MAX_INFLATE
# dspmap_box (dspmap_grow_boxes), the DSPMAP_BOX_* statuses and the DSPMAP_BOX_STOP_* causes (2 bits per face -x, +x, -y, +y, -z, +z in `stop`)
BOX_DTYPE = np.dtype([("lo", "i4", (3,)), ("hi", "i4", (3,)), ("status", "i4"), ("stop", "u4")])
BOX_OK, BOX_SEED_BLOCKED, BOX_SEED_OUTSIDE, BOX_INVALID = 0, 1, 3, 4
BOX_STOP_OBSTACLE, BOX_STOP_EDGE, BOX_STOP_LIMIT = 1, 2, 3
BOX_MAX_GROW = 64        # DSPMAP_BOX_MAX_GROW
BOX_WITH_CURRENT = 2     # DSPMAP_BOX_WITH_CURRENT
# dspmap_reach_point (dspmap_build_reach_fields, dspmap_reach_paths) and the DSPMAP_REACH_* constants
REACH_POINT_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("field", "i4")])
REACH_MAX_FIELDS = 64        # DSPMAP_REACH_MAX_FIELDS
REACH_MAX_STEPS = 4096       # DSPMAP_REACH_MAX_STEPS
REACH_UNREACHED = 65535      # DSPMAP_REACH_UNREACHED
REACH_WITH_CURRENT = 2       # DSPMAP_REACH_WITH_CURRENT
REACH_DEVICE_SETS = 4        # DSPMAP_REACH_DEVICE_SETS
REACH_TIMELINE_MAX_BYTES = 1 << 30   # DSPMAP_REACH_TIMELINE_MAX_BYTES
# dspmap_cost_bands (dspmap_build_cost_fields) and the DSPMAP_COST_* constants
COST_MAX_BANDS = 4           # DSPMAP_COST_MAX_BANDS
COST_MAX_WEIGHT = 8          # DSPMAP_COST_MAX_WEIGHT
COST_MAX_FIELDS = 64         # DSPMAP_COST_MAX_FIELDS
COST_MAX_COST = 16384        # DSPMAP_COST_MAX_COST
COST_UNREACHED = 65535       # DSPMAP_COST_UNREACHED


class CostBands(C.Structure):
    _fields_ = [("n_bands", C.c_int), ("clearance", C.c_float * 4), ("penalty", C.c_int * 4)]


# dspmap_path_info (dspmap_shorten_paths)
PATH_INFO_DTYPE = np.dtype([("n_cells", "i4"), ("n_segments", "i4"), ("n_blocked", "i4"), ("truncated", "i4")])
SHORTEN_MAX_WINDOW = 64      # DSPMAP_SHORTEN_MAX_WINDOW
FORECAST_MAX_TIMES = 64      # DSPMAP_FORECAST_MAX_TIMES
FORECAST_LERP = 2            # DSPMAP_FORECAST_LERP
# dspmap_view / dspmap_view_score (dspmap_score_views) and the DSPMAP_VIEW_* statuses
VIEW_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("qw", "f4"), ("qx", "f4"), ("qy", "f4"), ("qz", "f4"), ("max_range", "f4"), ("t", "f4")])
VIEW_SCORE_DTYPE = np.dtype([("n_seen", "i4"), ("n_unknown", "i4"), ("n_returns", "i4"), ("status", "i4")])
VIEW_OK, VIEW_BLOCKED, VIEW_OUTSIDE, VIEW_INVALID = 0, 1, 3, 4
# dspmap_view_set_score (dspmap_score_view_sets), dspmap_view_pick (dspmap_select_views) and their limits
VIEW_SET_SCORE_DTYPE = np.dtype([("n_seen", "i4"), ("n_unknown", "i4"), ("n_ok", "i4"), ("reserved", "i4")])
VIEW_PICK_DTYPE = np.dtype([("view", "i4"), ("gain", "i4"), ("covered", "i4"), ("reserved", "i4")])
VIEW_MAX_PICKS = 64                 # DSPMAP_VIEW_MAX_PICKS
VIEW_MASK_MAX_BYTES = 1 << 30       # DSPMAP_VIEW_MASK_MAX_BYTES
# dspmap_frontier_block (dspmap_build_frontiers)
FRONTIER_BLOCK_DTYPE = np.dtype([("block", "i4"), ("count", "i4"), ("sum_x", "i4"), ("sum_y", "i4"), ("sum_z", "i4"), ("unknown_faces", "i4")])
FRONTIER_MAX_BLOCK = 32
# dspmap_object (dspmap_build_objects): 88 bytes
OBJECT_DTYPE = np.dtype([("label", "i4"), ("count", "i4"), ("min_x", "i4"), ("max_x", "i4"), ("min_y", "i4"), ("max_y", "i4"), ("min_z", "i4"), ("max_z", "i4"),
                         ("sum_x", "i8"), ("sum_y", "i8"), ("sum_z", "i8"), ("mass_q", "i8"), ("mom_q", "i8", (3,))])
OBJECTS_MAX = 1 << 20        # the largest max_objects
OBJECT_Q = 1048576.0         # mass_q and mom_q count units of 2^-20
# dspmap_track (dspmap_track_update): 72 bytes
TRACK_DTYPE = np.dtype([("id", "i8"), ("parent", "i8"), ("prev_sum_x", "i8"), ("prev_sum_y", "i8"), ("prev_sum_z", "i8"), ("prev_count", "i4"),
                        ("prev_ordinal", "i4"), ("age", "i4"), ("born_seq", "i4"), ("overlap", "i4"), ("shift_x", "i4"), ("shift_y", "i4"), ("shift_z", "i4")])
TRACK_PER_CELL = 1           # DSPMAP_TRACK_PER_CELL
TRACK_MAX_SHIFT = 64         # the largest max_shift

# every symbol include/dspmap.h declares: name -> (restype, argtypes)
_P, _f, _i, _d = C.c_void_p, C.c_float, C.c_int, C.c_double
_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)
SIGNATURES = {
    "dspmap_default_config": (None, [C.POINTER(Config)]),
    "dspmap_create": (_P, [C.POINTER(Config)]),
    "dspmap_destroy": (None, [_P]),
    "dspmap_init_device": (_i, [_P]),
    "dspmap_last_error": (C.c_char_p, [_P]),
    "dspmap_sync": (_i, [_P]),
    "dspmap_set_stream": (_i, [_P, _P]),
    "dspmap_get_stream": (_P, [_P]),
    "dspmap_set_param": (_i, [_P, _i, _d]),
    "dspmap_get_param": (_d, [_P, _i]),
    "dspmap_set_gaussian_tables": (_i, [_P, _P, _P, _i]),
    "dspmap_set_rand_table": (_i, [_P, _P, _i]),
    "dspmap_set_cursors": (_i, [_P, _i, _i, _i]),
    "dspmap_get_cursors": (_i, [_P, _ip, _ip, _ip]),
    "dspmap_update": (_i, [_P, _i, _i, _P, _f, _f, _f, _d, _f, _f, _f, _f]),
    "dspmap_update_device": (_i, [_P, _i, _P, _i, _P, _P, _d, _P]),
    "dspmap_set_birth_cloud": (_i, [_P, _P, _i]),
    "dspmap_get_birth_cloud": (_i, [_P, _P, _i, _ip]),
    "dspmap_get_occupancy": (_i, [_P, _f, _P, _i, _ip]),
    "dspmap_get_occupancy_with_future": (_i, [_P, _f, _P, _i, _ip, _P]),
    "dspmap_get_future": (_i, [_P, _P]),
    "dspmap_clear_future": (_i, [_P]),
    "dspmap_get_results": (_i, [_P, _P]),
    "dspmap_results_device": (_P, [_P]),
    "dspmap_future_device": (_P, [_P]),
    "dspmap_query_occupancy": (_i, [_P, _i, _P, _f, _i, _f, _P]),
    "dspmap_query_occupancy_device": (_i, [_P, _i, _P, _f, _i, _f, _P]),
    "dspmap_trajectory_risk": (_i, [_P, _i, _i, _P, _f, _i, _f, _f, _P]),
    "dspmap_trajectory_risk_device": (_i, [_P, _i, _i, _P, _f, _i, _f, _f, _P]),
    "dspmap_build_distance_field": (_i, [_P, _f, _i, _i]),
    "dspmap_distance_field_device": (_P, [_P]),
    "dspmap_get_distance_field": (_i, [_P, _i, _P]),
    "dspmap_query_distance": (_i, [_P, _i, _P, _i, _f, _P, _P]),
    "dspmap_query_distance_device": (_i, [_P, _i, _P, _i, _f, _P, _P]),
    "dspmap_build_nearest_field": (_i, [_P, _f, _i, _i]),
    "dspmap_nearest_field_device": (_P, [_P]),
    "dspmap_nearest_distance_device": (_P, [_P]),
    "dspmap_get_nearest_field": (_i, [_P, _i, _P, _P]),
    "dspmap_query_nearest": (_i, [_P, _i, _P, _i, _f, _P]),
    "dspmap_query_nearest_device": (_i, [_P, _i, _P, _i, _f, _P]),
    "dspmap_build_cast_grid": (_i, [_P, _f, _i, _i]),
    "dspmap_cast_grid_device": (_P, [_P]),
    "dspmap_get_cast_grid": (_i, [_P, _i, _P]),
    "dspmap_cast_segments": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_cast_segments_device": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_grow_boxes": (_i, [_P, _i, _P, _P, _i, _P]),
    "dspmap_grow_boxes_device": (_i, [_P, _i, _P, _P, _i, _P]),
    "dspmap_build_reach_fields": (_i, [_P, _i, _i, _P, _f, _f, _i, _i]),
    "dspmap_build_reach_fields_device": (_i, [_P, _i, _i, _P, _f, _f, _i, _i]),
    "dspmap_reach_fields_device": (_P, [_P]),
    "dspmap_get_reach_field": (_i, [_P, _i, _P]),
    "dspmap_reach_paths": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_reach_paths_device": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_debug_reach_storage": (_i, [_P, _P]),
    "dspmap_build_reach_timeline": (_i, [_P, _i, _i, _P, _f, _f, _i, _i]),
    "dspmap_build_reach_timeline_device": (_i, [_P, _i, _i, _P, _f, _f, _i, _i]),
    "dspmap_reach_timeline_device": (_P, [_P]),
    "dspmap_reach_last_steps": (_i, [_P, _P]),
    "dspmap_get_reach_sets": (_i, [_P, _i, _i, _i, _P]),
    "dspmap_reach_timeline_paths": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_reach_timeline_paths_device": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_debug_set_cast_grid": (_i, [_P, _P]),
    "dspmap_build_cost_fields": (_i, [_P, _i, _i, _P, _f, _P, _i, _i]),
    "dspmap_build_cost_fields_device": (_i, [_P, _i, _i, _P, _f, _P, _i, _i]),
    "dspmap_cost_fields_device": (_P, [_P]),
    "dspmap_get_cost_field": (_i, [_P, _i, _P]),
    "dspmap_cost_weights_device": (_P, [_P]),
    "dspmap_get_cost_weights": (_i, [_P, _P]),
    "dspmap_cost_paths": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_cost_paths_device": (_i, [_P, _i, _P, _i, _i, _P, _P]),
    "dspmap_debug_set_distance_field": (_i, [_P, _P]),
    "dspmap_shorten_paths": (_i, [_P, _i, _i, _P, _P, _f, _f, _i, _i, _i, _P, _P, _P]),
    "dspmap_shorten_paths_device": (_i, [_P, _i, _i, _P, _P, _f, _f, _i, _i, _i, _P, _P, _P]),
    "dspmap_build_forecast": (_i, [_P, _i, _P, _i]),
    "dspmap_forecast_device": (_P, [_P]),
    "dspmap_forecast_times": (_i, [_P, _P, _i]),
    "dspmap_get_forecast": (_i, [_P, _i, _P]),
    "dspmap_query_forecast": (_i, [_P, _i, _P, _i, _f, _P]),
    "dspmap_query_forecast_device": (_i, [_P, _i, _P, _i, _f, _P]),
    "dspmap_known_integrate": (_i, [_P, _f, _i]),
    "dspmap_known_reset": (_i, [_P]),
    "dspmap_get_known": (_i, [_P, _P]),
    "dspmap_query_known": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_query_known_device": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_mask_cast_grid": (_i, [_P, _i, _i]),
    "dspmap_known_stats": (_i, [_P, _i, _P]),
    "dspmap_get_view": (_i, [_P, _P, _P, _P]),
    "dspmap_score_views": (_i, [_P, _i, _P, _i, _i, _P]),
    "dspmap_score_views_device": (_i, [_P, _i, _P, _i, _i, _P]),
    "dspmap_score_view_sets": (_i, [_P, _i, _i, _P, _i, _i, _P, _P]),
    "dspmap_score_view_sets_device": (_i, [_P, _i, _i, _P, _i, _i, _P, _P]),
    "dspmap_select_views": (_i, [_P, _i, _P, _i, _i, _i, _i, _i, _P, _P]),
    "dspmap_select_views_device": (_i, [_P, _i, _P, _i, _i, _i, _i, _i, _P, _P]),
    "dspmap_view_rays": (_i, [_P, _P, _P, _P, _P]),
    "dspmap_debug_view_cells": (_i, [_P, _P, _i, _P, _P]),
    "dspmap_build_frontiers": (_i, [_P, _f, _i, _i, _i, _i]),
    "dspmap_frontier_counts": (_i, [_P, _P]),
    "dspmap_get_frontier_grid": (_i, [_P, _P]),
    "dspmap_get_frontier_cells": (_i, [_P, _i, _P, _P]),
    "dspmap_get_frontier_blocks": (_i, [_P, _i, _P, _P]),
    "dspmap_frontier_grid_device": (_P, [_P]),
    "dspmap_frontier_cells_device": (_P, [_P]),
    "dspmap_frontier_blocks_device": (_P, [_P]),
    "dspmap_frontier_counts_device": (_P, [_P]),
    "dspmap_debug_set_known": (_i, [_P, _P]),
    "dspmap_build_objects": (_i, [_P, _f, _i, _i, _i, _i]),
    "dspmap_object_counts": (_i, [_P, _P]),
    "dspmap_get_objects": (_i, [_P, _i, _P, _P]),
    "dspmap_get_object_labels": (_i, [_P, _P]),
    "dspmap_objects_device": (_P, [_P]),
    "dspmap_object_labels_device": (_P, [_P]),
    "dspmap_object_counts_device": (_P, [_P]),
    "dspmap_query_objects": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_query_objects_device": (_i, [_P, _i, _P, _i, _P]),
    "dspmap_track_update": (_i, [_P, _f, _i, _i, _i, _i]),
    "dspmap_track_reset": (_i, [_P]),
    "dspmap_track_counts": (_i, [_P, _P]),
    "dspmap_get_tracks": (_i, [_P, _i, _P, _P]),
    "dspmap_tracks_device": (_P, [_P]),
    "dspmap_track_counts_device": (_P, [_P]),
    "dspmap_voxel_center": (None, [_P, _i, _fp, _fp, _fp]),
    "dspmap_point_voxel_index": (_i, [_P, _f, _f, _f, _ip]),
    "dspmap_voxel_num": (_i, [_P]),
    "dspmap_local_voxel_num": (_i, [_P]),
    "dspmap_local_voxel_base": (_i, [_P]),
    "dspmap_slots_per_voxel": (_i, [_P]),
    "dspmap_pyramid_num": (_i, [_P]),
    "dspmap_pyramid_capacity": (_i, [_P]),
    "dspmap_get_counters": (_i, [_P, C.POINTER(Counters)]),
    "dspmap_set_profiling": (_i, [_P, _i]),
    "dspmap_get_stage_ms": (_i, [_P, _fp, _ip]),
    "dspmap_get_event_overhead_ms": (_i, [_P, _fp]),
    "dspmap_debug_stream": (_i, [_P, _i, C.POINTER(C.c_longlong)]),
    "dspmap_debug_sweep_probe": (_i, [_P, _i, _i, _i, _i, _fp, C.POINTER(C.c_longlong)]),
    "dspmap_debug_tile_view": (_i, [_P, C.POINTER(C.c_int), _i]),
    "dspmap_debug_rollout_paths": (_i, [_P, C.POINTER(C.c_longlong)]),
    "dspmap_debug_rollout_plan": (_i, [_P, _ip, _ip]),
    "dspmap_debug_pair_items": (_i, [_P, _ip]),
    "dspmap_debug_weight_variant": (_i, [_P]),
    "dspmap_debug_pair_path": (_i, [_P]),
    "dspmap_debug_estimator_queue": (_i, [_P, C.POINTER(C.c_longlong)]),
    "dspmap_debug_frame_branches": (_i, [_P, C.POINTER(C.c_longlong)]),
    "dspmap_debug_resample_split_frames": (C.c_longlong, [_P]),
    "dspmap_debug_plain_frames": (C.c_longlong, [_P]),
    "dspmap_debug_estimator_path": (_i, [_P]),
    "dspmap_debug_tile_count": (_i, [_P]),
    "dspmap_debug_tile_of_voxels": (_i, [_P, _i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dspmap_debug_tile_moving": (_i, [_P, C.POINTER(C.c_int), _i]),
    "dspmap_debug_rdzv_publish": (_i, [C.c_char_p, C.c_char_p]),
    "dspmap_debug_rdzv_wait": (_i, [C.c_char_p, _i, C.c_char_p]),
    "dspmap_clear_state": (_i, [_P]),
    "dspmap_import_state": (_i, [_P, _i, _P, _P, _P]),
    "dspmap_export_state": (_i, [_P, _i, _P, _P, _P, _ip]),
    "dspmap_save_checkpoint": (_i, [_P, C.c_char_p]),
    "dspmap_load_checkpoint": (_i, [_P, C.c_char_p]),
    "dspmap_preprocess_cloud": (_i, [_P, _i, _P, _i, _f, _i, _i, _P, _ip, _ip]),
    "dspmap_preprocess_depth": (_i, [_P, C.POINTER(Camera), _P, _f, _i, _P, _ip, _ip, _ip]),
    "dspmap_update_depth_device": (_i, [_P, C.POINTER(Camera), _P, _f, _i, _P, _d, _P]),
    "dspmap_update_depth": (_i, [_P, C.POINTER(Camera), _P, _f, _i, _P, _d, _P]),
    "dspmap_add_random_particles": (_i, [_P, _i, _f]),
    "dspmap_seed_uniform_moving": (_i, [_P, _i, _f, C.c_uint, _f]),
    "dspmap_seed_uniform": (_i, [_P, _i, _f, C.c_uint]),
    "dspmap_stage_bin_points": (_i, [_P, _i, _i, _P, _f, _f, _f, _f]),
    "dspmap_set_current_position": (_i, [_P, _f, _f, _f]),
    "dspmap_stage_predict": (_i, [_P, _f, _f, _f, _f]),
    "dspmap_stage_update": (_i, [_P]),
    "dspmap_stage_birth": (_i, [_P]),
    "dspmap_stage_resample": (_i, [_P]),
    "dspmap_get_observations": (_i, [_P, _P, _P, _P, _fp]),
    "dspmap_set_expected_newborn": (_i, [_P, _f]),
    "dspmap_get_pyramid_counts": (_i, [_P, _P]),
    "dspmap_get_pyramid_candidates": (_i, [_P, _P]),
    "dspmap_mgpu_bind": (_i, [_P, _P, _P, _i]),
    "dspmap_mgpu_place_interior": (_i, [_P]),
    "dspmap_mgpu_begin": (_i, [_P, _i, _P, _i, _P, _P, _d, _P]),
    "dspmap_mgpu_export": (_i, [_P, _i, _P, _i, _ip]),
    "dspmap_mgpu_export_both": (_i, [_P, _P, _P, _i, _P]),
    "dspmap_mgpu_set_export_counts": (_i, [_P, _i, _i]),
    "dspmap_mgpu_import": (_i, [_P, _i, _P]),
    "dspmap_mgpu_ck_partial": (_i, [_P]),
    "dspmap_mgpu_weights_and_split": (_i, [_P]),
    "dspmap_mgpu_finish": (_i, [_P]),
    "dspmap_mgpu_get_unique_id": (_i, [_P]),
    "dspmap_mgpu_comm_init": (_i, [_P, _i, _i, _P]),
    "dspmap_mgpu_comm_init_from_env": (_i, [_P]),
    "dspmap_mgpu_comm_destroy": (_i, [_P]),
    "dspmap_mgpu_update": (_i, [_P, _i, _P, _i, _P, _P, _d, _P]),
    "dspmap_mgpu_update_host": (_i, [_P, _i, _i, _P, _f, _f, _f, _d, _f, _f, _f, _f]),
    "dspmap_mgpu_message_records": (_i, [_P]),
    "dspmap_mgpu_group_create": (_i, [_P, _i]),
    "dspmap_mgpu_group_update": (_i, [_P, _i, _i, _P, _i, _P, _P, _d, _P]),
    "dspmap_mgpu_group_set_profiling": (_i, [_P, _i, _i]),
    "dspmap_mgpu_group_get_phase_ms": (_i, [_P, _i, _fp, _ip]),
}

_LIB = None


def load_library(path=None):
    """dlopen the HIP library and bind every declared symbol.  Raises if it is missing."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            "%s not found: build it with `python dsp-map_amd/build_ext.py` (hipcc, gfx950). "
            "There is no CPU fallback." % p)
    # Load order matters in a process that also uses PyTorch-ROCm: torch ships its own copy of the HIP / HSA
    # runtime, and the copy that is initialised first owns the device; a second one then reports "no device".
    # Import torch (when it is installed) BEFORE this library so that both share torch's runtime, whatever
    # order the caller imports things in.  A process without torch is unaffected.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001
        pass
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _LIB = lib
    return lib


def make_config(nx=66, ny=66, nz=40, res=0.15, ppv=9, angle=3, half_fov_h=42, half_fov_v=24,
                pred_times=(0.05, 0.2, 0.5, 1.0, 1.5, 2.0), z_lo=0, z_hi=0, device=-1,
                table_size=0, seed=0, neighbor_n=0, safe_factor=0, static_model=0):
    c = Config()
    c.pyramid_neighbor_n, c.safe_particle_factor, c.static_model = neighbor_n, safe_factor, static_model
    c.nx, c.ny, c.nz = nx, ny, nz
    c.voxel_resolution = res
    c.angle_resolution = angle
    c.max_particle_num_voxel = ppv
    c.half_fov_h, c.half_fov_v = half_fov_h, half_fov_v
    c.prediction_times = len(pred_times)
    for k, t in enumerate(pred_times):
        c.prediction_future_time[k] = t
    c.z_lo, c.z_hi = z_lo, z_hi
    c.device = device
    c.gaussian_table_size = table_size
    c.seed = seed
    return c


class DSPMapError(RuntimeError):
    pass


class _DeviceSpan:
    """device memory the library owns, for torch.as_tensor: the CUDA array interface, which torch wraps without a copy"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class DSPMap:
    """Mirror of the reference's DSPMap (dsp_dynamic.h:142) on top of the C ABI."""

    def __init__(self, cfg=None, example_params=True, init_particle_num=0, init_weight=0.01):
        self.L = load_library()
        self.cfg = cfg or make_config()
        self.h = self.L.dspmap_create(C.byref(self.cfg))
        if not self.h:
            raise DSPMapError("dspmap_create rejected the configuration")
        self.V = self.L.dspmap_voxel_num(self.h)
        self.V_local = self.L.dspmap_local_voxel_num(self.h)
        self.slots = self.L.dspmap_slots_per_voxel(self.h)
        self.NP = self.L.dspmap_pyramid_num(self.h)
        self.capp = self.L.dspmap_pyramid_capacity(self.h)
        self.T = self.cfg.prediction_times
        if example_params:  # src/map_sim_example.cpp:522-526
            self.setPredictionVariance(0.05, 0.05)
            self.setObservationStdDev(0.1)
            self.setNewBornParticleNumberofEachPoint(20)
            self.setNewBornParticleWeight(0.0001)
            self.setOriginalVoxelFilterResolution(0.1)
        if init_particle_num:
            self._chk(self.L.dspmap_add_random_particles(self.h, init_particle_num, init_weight))

    # -- plumbing
    def _chk(self, rc):
        if rc < 0:
            raise DSPMapError(self.L.dspmap_last_error(self.h).decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.dspmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._chk(self.L.dspmap_sync(self.h))

    def set_param(self, key, value):
        self._chk(self.L.dspmap_set_param(self.h, key, float(value)))

    def get_param(self, key):
        return self.L.dspmap_get_param(self.h, key)

    def rollout_paths(self):
        """(variant, adds through k_rollout's LDS windows, single-atomic adds of k_rollout) of the last resampling stage;
        variant: bit 0 = k_resample_wg, bits 1-2 = rollout 0 inline / 1 k_rollout light / 2 k_rollout windows / 3 none"""
        out = (C.c_longlong * 3)()
        self._chk(self.L.dspmap_debug_rollout_paths(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def rollout_plan(self):
        """(halo rows per horizon of k_rollout's LDS windows, LDS cells of all windows) for this handle; all halos 0 = the collapsed plan"""
        halo = (C.c_int * MAX_PRED)()
        cells = C.c_int()
        n = self._chk(self.L.dspmap_debug_rollout_plan(self.h, halo, C.byref(cells)))
        return [int(halo[t]) for t in range(n)], cells.value

    def pair_items(self):
        """(work items of k_ck_partial, work items of k_weight, particles per k_ck_partial item) of the last weight update"""
        out = (C.c_int * 3)()
        self._chk(self.L.dspmap_debug_pair_items(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def weight_variant(self):
        """which k_weight the last weight update launched: 'mask' (every pair evaluated), 'skip' (far pairs branched over), or None"""
        return {0: None, 1: "mask", 2: "skip"}.get(self.L.dspmap_debug_weight_variant(self.h))

    def pair_path(self):
        """how the last frame gave its pair kernels their work: 'prepared' (k_pyr_prepare), 'self' (self-mapped, no k_pyr_prepare), or None
        -- DSPMAP_P_PAIR_PREPARE"""
        return {0: None, 1: "prepared", 2: "self"}.get(self.L.dspmap_debug_pair_path(self.h))

    def estimator_queue(self):
        """(frames whose estimator ran on a queue of its own, hand-over word 0, hand-over word 1, give-ups, frames whose first birth kernel
        had to wait for the birth cloud, shares its workgroup 0 did for the others) -- DSPMAP_P_ESTIMATOR_QUEUE"""
        out = (C.c_longlong * 6)()
        self._chk(self.L.dspmap_debug_estimator_queue(self.h, out))
        return tuple(int(v) for v in out)

    def frame_branches(self):
        """(frames run as two branches, tiles of class Q, tiles of class P, tiles of the map, largest speed ever given in mm/s) -- DSPMAP_P_FRAME_BRANCHES"""
        out = (C.c_longlong * 5)()
        self._chk(self.L.dspmap_debug_frame_branches(self.h, out))
        return tuple(int(v) for v in out)

    def resample_split_frames(self):
        """frames whose resampling stage ran as two launches -- DSPMAP_P_RESAMPLE_SPLIT"""
        return int(self.L.dspmap_debug_resample_split_frames(self.h))

    def plain_frames(self):
        """frames queued as plain launches with their parameter block in the pinned ring -- DSPMAP_P_USE_GRAPH"""
        return int(self.L.dspmap_debug_plain_frames(self.h))

    def estimator_path(self):
        """where the last device-estimator frame ran the estimator: 'own_stream', 'forked_shared_queue' (the fallback), 'forked', or None"""
        return {0: None, 1: "own_stream", 2: "forked_shared_queue", 3: "forked"}.get(self.L.dspmap_debug_estimator_path(self.h))

    def tile_count(self):
        return self.L.dspmap_debug_tile_count(self.h)

    def tile_of(self, voxels):
        """the 64-voxel tile each of the given GLOBAL voxel indices lives in (runs of 64 indices or 4x4x4 cubes: DSPMAP_P_TILING)"""
        import numpy as np
        v = np.ascontiguousarray(voxels, np.int32)
        out = np.zeros(v.size, np.int32)
        self._chk(self.L.dspmap_debug_tile_of_voxels(self.h, v.size, v.ctypes.data_as(C.POINTER(C.c_int)), out.ctypes.data_as(C.POINTER(C.c_int))))
        return out

    def tile_moving(self):
        """per 64-voxel tile: 0 = all of its live particles are static (its velocity rows are not fetched by the sweeps)"""
        import numpy as np
        n = self.tile_count()
        out = np.zeros(n, np.int32)
        r = self.L.dspmap_debug_tile_moving(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), n)
        if r < 0:
            self._chk(r)
        return out[:r]

    # -- reference setters (dsp_dynamic.h:355-382)
    def setPredictionVariance(self, p_stddev, v_stddev):
        self.set_param(P_POSITION_STDDEV, p_stddev)
        self.set_param(P_VELOCITY_STDDEV, v_stddev)
        self.set_param(P_REGENERATE_TABLES, 1)

    def setObservationStdDev(self, s):
        self.set_param(P_OBSERVATION_STDDEV, s)

    def setNewBornParticleWeight(self, w):
        self.set_param(P_NEWBORN_WEIGHT, w)

    def setNewBornParticleNumberofEachPoint(self, n):
        self.set_param(P_NEWBORN_NUMBER, n)

    def setOriginalVoxelFilterResolution(self, r):
        self.set_param(P_VOXEL_FILTER_RES, r)

    def useVelocityEstimator(self, on):
        self.set_param(P_VELOCITY_ESTIMATOR, 1 if on else 0)

    # -- randomness
    def set_tables(self, p_tab, v_tab, rand_ints=None):
        p_tab = np.ascontiguousarray(p_tab, np.float32)
        v_tab = np.ascontiguousarray(v_tab, np.float32)
        self._chk(self.L.dspmap_set_gaussian_tables(self.h, _ptr(p_tab), _ptr(v_tab), p_tab.size))
        if rand_ints is not None:
            r = np.ascontiguousarray(rand_ints, np.int32)
            self._chk(self.L.dspmap_set_rand_table(self.h, _ptr(r), r.size))

    def cursors(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.dspmap_get_cursors(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_cursors(self, p_cursor=-1, v_cursor=-1, r_cursor=-1):
        """move the cursors of the position / velocity / rand() tables; a negative value leaves that cursor where it is"""
        self._chk(self.L.dspmap_set_cursors(self.h, int(p_cursor), int(v_cursor), int(r_cursor)))

    # -- the frame (dsp_dynamic.h:181)
    def update(self, pts, pos, stamp, quat):
        """pts: (n,3) float32 host array, sensor frame.  Returns 1 (ok) / 0 (rejected)."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        return self._chk(self.L.dspmap_update(self.h, pts.shape[0], 3, _ptr(pts), pos[0], pos[1], pos[2],
                                              float(stamp), quat[0], quat[1], quat[2], quat[3]))

    def update_device(self, pts_dev_ptr, n, pos, stamp, quat, birth_dev_ptr=None, n_birth=0):
        pos_a = (C.c_float * 3)(*pos)
        q_a = (C.c_float * 4)(*quat)
        return self._chk(self.L.dspmap_update_device(self.h, n, pts_dev_ptr, n_birth, birth_dev_ptr,
                                                     C.cast(pos_a, C.c_void_p), float(stamp),
                                                     C.cast(q_a, C.c_void_p)))

    def set_birth_cloud(self, vpts):
        vpts = np.ascontiguousarray(vpts, VPOINT_DTYPE)
        self._chk(self.L.dspmap_set_birth_cloud(self.h, _ptr(vpts), vpts.size))

    def get_birth_cloud(self):
        n = C.c_int()
        self._chk(self.L.dspmap_get_birth_cloud(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, VPOINT_DTYPE)
        if n.value:
            self._chk(self.L.dspmap_get_birth_cloud(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    # -- readout (dsp_dynamic.h:385-438)
    def getOccupancyMap(self, threshold=0.7):
        xyz = np.zeros((self.V_local, 3), np.float32)
        n = C.c_int()
        self._chk(self.L.dspmap_get_occupancy(self.h, threshold, _ptr(xyz), self.V_local, C.byref(n)))
        return n.value, xyz[:n.value].copy()

    def getOccupancyMapWithFutureStatus(self, threshold=0.7):
        xyz = np.zeros((self.V_local, 3), np.float32)
        fut = np.zeros((self.V_local, self.T), np.float32)
        n = C.c_int()
        self._chk(self.L.dspmap_get_occupancy_with_future(self.h, threshold, _ptr(xyz), self.V_local,
                                                          C.byref(n), _ptr(fut)))
        return n.value, xyz[:n.value].copy(), fut

    def getFutureStatus(self):
        fut = np.zeros((self.V_local, self.T), np.float32)
        self._chk(self.L.dspmap_get_future(self.h, _ptr(fut)))
        return fut

    def clearOccupancyMapPrediction(self):
        self._chk(self.L.dspmap_clear_future(self.h))

    def results(self):
        """[V_local, 4]: occupancy mass, mean vx, vy, vz (voxels_objects_number[v][0..3])."""
        out = np.zeros((self.V_local, 4), np.float32)
        self._chk(self.L.dspmap_get_results(self.h, _ptr(out)))
        return out

    # -- point / trajectory queries (extension; semantics in include/dspmap.h next to dspmap_query_occupancy)
    @staticmethod
    def _is_device_tensor(a):
        return type(a).__module__.startswith("torch") and getattr(a, "is_cuda", False)

    @staticmethod
    def _device_samples(q, shape_tail, what):
        import torch
        if q.dtype != torch.float32 or tuple(q.shape[-len(shape_tail):]) != shape_tail:
            raise ValueError("%s: a float32 tensor of shape %s" % (what, "[..., " + ", ".join(map(str, shape_tail)) + "]"))
        return q.contiguous()

    def _handle_stream_order(self, dev):
        """(before, after) for a device call: when the handle queues on a stream other than torch's current one, `before` makes the
        handle's stream wait for the work torch has queued so far (the samples), `after` makes torch's stream wait for the query.
        So the result is ordered for torch's consumers, and the samples (also a temporary made by .contiguous()) and the output,
        allocated on torch's stream, are not handed out again by the caching allocator before the handle has used them.  Both waits
        are queued at once (no reference to the handle's stream outlives the call); no host synchronisation."""
        import torch
        cur = torch.cuda.current_stream(dev)
        s = self.L.dspmap_get_stream(self.h) or 0
        if s == cur.cuda_stream:
            return (lambda: None), (lambda: None)
        ext = torch.cuda.ExternalStream(s, device=dev)
        return (lambda: ext.wait_stream(cur)), (lambda: cur.wait_stream(ext))

    # -- the one call path of the planning layers: every wrapper below states its inputs, outputs and flags and goes through these
    def _input(self, a, width, what, want=None, ndim=None):
        """(input made contiguous, its rows, its torch device or None for numpy) of rows of `width` numbers: float32 rows described by
        `want` (the shape in the ValueError, `ndim` dimensions where that is fixed), or with want=None dspmap_reach_point rows.  The
        only place that tells a GPU tensor from host data."""
        dev = a.device if self._is_device_tensor(a) else None
        if want is None:
            q = self._reach_points(a, what) if dev is None else self._reach_points_device(a, what)
            return q, (len(q) if dev is None else q.numel() // 4), dev
        if dev is not None:
            q = self._device_samples(a, (width,), what)
            if ndim is not None and q.dim() != ndim:
                raise ValueError("%s: %s" % (what, want))
            return q, q.numel() // width, dev
        q = np.ascontiguousarray(a, np.float32)
        if (ndim is not None and q.ndim != ndim) or q.shape[-1:] != (width,):
            raise ValueError("%s: %s" % (what, want))
        return q, q.size // width, None

    @staticmethod
    def _alloc(dev, shape, dtype):
        """an output where the input is: zeroed numpy of `dtype`, or an uninitialised tensor on `dev` -- float32 / int32, a structured
        dtype as its int32 columns"""
        if dev is None:
            return np.zeros(shape, dtype)
        import torch
        dtype = np.dtype(dtype)
        shape = shape if isinstance(shape, tuple) else (shape,)
        if dtype.names:
            return torch.empty(shape + (dtype.itemsize // 4,), dtype=torch.int32, device=dev)
        return torch.empty(shape, dtype=torch.float32 if dtype == np.float32 else torch.int32, device=dev)

    @staticmethod
    def _p(a, when=True):
        """the pointer argument of an array, a tensor or None; NULL also where `when` does not hold"""
        if a is None or not when:
            return None
        return _ptr(a) if isinstance(a, np.ndarray) else a.data_ptr()

    def _call(self, dev, symbol, *args, init_device=False):
        """the host entry point `symbol` (dev None: synchronous), or `symbol`_device enqueued on the handle's stream and ordered with
        torch's current stream both ways; init_device: dspmap_init_device first (the handle's stream exists from there on).  An
        error raises before torch's stream is made to wait."""
        if dev is None:
            return self._chk(getattr(self.L, symbol)(self.h, *args))
        if init_device:
            self._chk(self.L.dspmap_init_device(self.h))
        before, after = self._handle_stream_order(dev)
        before()
        rc = self._chk(getattr(self.L, symbol + "_device")(self.h, *args))
        after()
        return rc

    @staticmethod
    def _fields(raw, dtype, dev):
        """a result of structured `dtype`: the numpy array as it is; the int32 block of a device call as a dict of views, one per field"""
        if dev is None:
            return raw
        import torch
        out = {}
        for name in dtype.names:
            ft, off = dtype.fields[name][:2]
            col = raw[:, off // 4:(off + ft.itemsize) // 4] if ft.shape else raw[:, off // 4]
            out[name] = col.view(torch.float32) if ft.base == np.float32 else col
        return out

    def _query(self, symbol, q, dtype, mid, init_device=False, grad=None):
        """one value of `dtype` per sample {x, y, z, t} of q: symbol(h, n, q, *mid, out[, grad]); grad None: the entry point takes none"""
        q, n, dev = self._input(q, 4, symbol[7:], "samples of shape [n, 4]")
        out = self._alloc(dev, n, dtype)
        g = self._alloc(dev, (n, 3), np.float32) if grad else None
        self._call(dev, symbol, n, self._p(q), *mid, self._p(out), *(() if grad is None else (self._p(g),)), init_device=init_device)
        return (out, g) if grad else out

    def _paths(self, symbol, starts, max_len, world):
        """reach_paths / reach_timeline_paths / cost_paths: (value [n] int32, cells [n, max_len] int32) from starts {x, y, z, field}.
        The host entry points get NULL for an empty input, the device ones the tensor's address."""
        max_len = int(max_len)
        q, n, dev = self._input(starts, 4, symbol[7:])
        value = self._alloc(dev, n, np.int32)
        cells = self._alloc(dev, (n, max(max_len, 0)), np.int32)
        some = n > 0 or dev is not None
        self._call(dev, symbol, n, self._p(q, some), max_len, QUERY_WORLD if world else 0, self._p(value, some), self._p(cells, max_len > 0))
        return value, cells

    def _layers(self, symbol, which, n_all, shape, dtype):
        """one layer / field of a grid as numpy `shape`, or with which=None the first n_all of them [n_all, *shape] (host copies)"""
        idx = range(int(n_all)) if which is None else [int(which)]
        out = np.zeros((len(idx),) + shape, dtype)
        for j, l in enumerate(idx):
            self._chk(getattr(self.L, symbol)(self.h, l, _ptr(out[j])))
        return out if which is None else out[0]

    def _counts(self, symbol, k, *args):
        """the k 64-bit counts symbol(h, *args, out) writes, as a tuple of ints"""
        out = (C.c_longlong * k)()
        self._chk(getattr(self.L, symbol)(self.h, *args, C.cast(out, C.c_void_p)))
        return tuple(int(v) for v in out)

    def _list(self, symbol, dtype, device=None, device_symbol=None):
        """the records of a list of the last build: asked for its length with no room (which synchronises the handle's stream and raises
        on a stale snapshot), then copied to numpy `dtype` [n] -- or with device= handed out in place as int32 columns"""
        n = C.c_int(0)
        self._chk(getattr(self.L, symbol)(self.h, 0, None, C.byref(n)))
        if device is not None:
            return self._span(device, device_symbol, (n.value, dtype.itemsize // 4))
        out = np.zeros(n.value, dtype)
        if n.value:
            self._chk(getattr(self.L, symbol)(self.h, n.value, _ptr(out), C.byref(n)))
        return out

    def _span(self, device, symbol, shape):
        """an int32 tensor of `shape` over the buffer symbol(h) names, without a copy, torch's current stream ordered behind the handle's;
        an empty tensor of its own where the shape holds nothing.  The caller has read the shape from a synchronised snapshot."""
        import torch
        dev = torch.device(device)
        _, after = self._handle_stream_order(dev)
        after()
        if 0 in shape:
            return torch.empty(shape, dtype=torch.int32, device=dev)
        return torch.as_tensor(_DeviceSpan(getattr(self.L, symbol)(self.h), shape, "<i4"), device=dev)

    def query_occupancy(self, q, radius=0.0, world=False, outside=1.0):
        """value of every sample {x, y, z, t} of q ([n, 4] float32): the maximum over the own voxel and the voxel centres within
        `radius` of the current mass (t < 0) or of the future status at the first horizon >= t, `outside` for what lies outside
        the map.  A numpy array goes through the host entry point (synchronous) and returns numpy; a torch tensor on the GPU goes
        through the device entry point: the result is a tensor on the same device, enqueued on the handle's stream and ordered
        with torch's current stream both ways (no host synchronisation; none needed when the handle is on torch's stream)."""
        return self._query("dspmap_query_occupancy", q, np.float32, (float(radius), QUERY_WORLD if world else 0, float(outside)), init_device=True)

    def trajectory_risk(self, samples, radius=0.0, world=False, outside=1.0, threshold=0.5):
        """per trajectory of samples ([K, S, 4] float32, trajectory-major): sequential fp32 sum, max, first sample > threshold (-1:
        none) and the samples outside the map of the values query_occupancy gives.  numpy in -> structured numpy (RISK_DTYPE) out
        (synchronous); a torch tensor on the GPU -> dict of tensors 'sum', 'max' (float32), 'first_over', 'n_outside' (int32) on the
        same device, enqueued on the handle's stream."""
        q, _, dev = self._input(samples, 4, "trajectory_risk", "samples of shape [K, S, 4]", ndim=3)
        k, s = int(q.shape[0]), int(q.shape[1])
        out = self._alloc(dev, k, RISK_DTYPE)
        self._call(dev, "dspmap_trajectory_risk", k, s, self._p(q), float(radius), QUERY_WORLD if world else 0, float(outside), float(threshold),
                   self._p(out), init_device=True)
        return self._fields(out, RISK_DTYPE, dev)

    # -- distance fields (extension; semantics in include/dspmap.h next to dspmap_build_distance_field)
    def build_distance_field(self, threshold, max_voxels, outside_occupied=False):
        """enqueue the truncated Euclidean distance fields of all T + 1 layers (0: current mass, 1 + k: horizon k) on the handle's stream:
        metres to the nearest voxel with mass > threshold, at most max_voxels voxels; outside_occupied counts the lattice just outside
        the map as occupied.  Read-only towards the map; the field is a snapshot and goes stale with the next frame."""
        self._chk(self.L.dspmap_build_distance_field(self.h, float(threshold), int(max_voxels), DIST_OUTSIDE_OCCUPIED if outside_occupied else 0))

    def distance_field(self, layer=None):
        """the field of one layer as numpy [nz, ny, nx], or of all layers [L, nz, ny, nx] (synchronous host copies)"""
        return self._layers("dspmap_get_distance_field", layer, self.T + 1, (self.cfg.nz, self.cfg.ny, self.cfg.nx), np.float32)

    def distance_field_ptr(self):
        """device address of the [L][V] float32 field, or None when there is none / it is stale"""
        return self.L.dspmap_distance_field_device(self.h) or None

    def query_distance(self, q, world=False, outside=0.0, grad=True):
        """distance (and gradient [n, 3] unless grad is False) of every sample {x, y, z, t} of q ([n, 4] float32) in the layer its t
        selects (t < 0: current, else the first horizon >= t): the field at the point's own voxel and its central / one-sided
        differences; `outside` and a zero gradient for what lies outside the map.  numpy in -> numpy out (synchronous); a torch tensor
        on the GPU -> tensors on the same device, enqueued on the handle's stream and ordered with torch's current stream like
        query_occupancy.  Returns (dist, grad) or dist."""
        return self._query("dspmap_query_distance", q, np.float32, (QUERY_WORLD if world else 0, float(outside)), grad=bool(grad))

    # -- nearest-obstacle fields (extension; semantics in include/dspmap.h next to dspmap_build_nearest_field)
    def build_nearest_field(self, threshold, max_voxels, signed=False, from_cast_grid=False):
        """enqueue the nearest-obstacle fields of all T + 1 layers on the handle's stream: per voxel the global index of the nearest
        occupied voxel within max_voxels voxels (ties: the smallest index; -1: none) and the distance to it in metres.  signed: an
        occupied voxel gets its nearest FREE voxel and a negative distance instead of itself and 0.  from_cast_grid: the occupied set
        is the valid cast grid as it is now (threshold is not read), else mass > threshold.  Read-only towards the map; a snapshot like
        the distance field, which also goes stale with the cast grid when built from it."""
        flags = (NEAREST_SIGNED if signed else 0) | (NEAREST_FROM_CAST_GRID if from_cast_grid else 0)
        self._chk(self.L.dspmap_build_nearest_field(self.h, float(threshold), int(max_voxels), flags))

    def _nearest_layers(self, layer, dtype, second):
        """_layers for the getter with two outputs: the first (int32 indices) or the second (float32 distances)"""
        idx = range(self.T + 1) if layer is None else [int(layer)]
        out = np.zeros((len(idx), self.cfg.nz, self.cfg.ny, self.cfg.nx), dtype)
        for j, l in enumerate(idx):
            self._chk(self.L.dspmap_get_nearest_field(self.h, l, None if second else _ptr(out[j]), _ptr(out[j]) if second else None))
        return out if layer is None else out[0]

    def nearest_field(self, layer=None):
        """the nearest-voxel indices of one layer as numpy int32 [nz, ny, nx], or of all layers [L, nz, ny, nx] (synchronous host copies)"""
        return self._nearest_layers(layer, np.int32, False)

    def nearest_distance(self, layer=None):
        """the (signed) distances of one layer as numpy float32 [nz, ny, nx], or of all layers [L, nz, ny, nx] (synchronous host copies)"""
        return self._nearest_layers(layer, np.float32, True)

    def nearest_field_ptr(self):
        """device address of the [L][V] int32 indices, or None when there are none / they are stale"""
        return self.L.dspmap_nearest_field_device(self.h) or None

    def nearest_distance_ptr(self):
        """device address of the [L][V] float32 distances, or None when there are none / they are stale"""
        return self.L.dspmap_nearest_distance_device(self.h) or None

    def query_nearest(self, q, world=False, outside=0.0):
        """the nearest obstacle of every sample {x, y, z, t} of q ([n, 4] float32) in the layer its t selects: the own voxel's distance
        and nearest voxel, the offset from the point to that voxel's centre and, in the current layer, the velocity of the occupied
        voxel of the pair; {outside, -1, 0 ...} for what lies outside the map.  numpy in -> structured numpy (NEAREST_DTYPE: dist, voxel,
        offset[3], velocity[3]) out, synchronous; a torch tensor on the GPU -> dict of tensors 'dist' (float32), 'voxel' (int32),
        'offset', 'velocity' ([n, 3] float32) on the same device, enqueued on the handle's stream and ordered with torch's current
        stream like query_occupancy."""
        q, n, dev = self._input(q, 4, "query_nearest", "samples of shape [n, 4]")
        out = self._alloc(dev, n, NEAREST_DTYPE)
        self._call(dev, "dspmap_query_nearest", n, self._p(q), QUERY_WORLD if world else 0, float(outside), self._p(out))
        return self._fields(out, NEAREST_DTYPE, dev)

    # -- segment casts (extension; semantics in include/dspmap.h next to dspmap_build_cast_grid)
    def build_cast_grid(self, threshold, inflate_voxels=0):
        """enqueue the bit grids of all T + 1 layers (0: current mass, 1 + k: horizon k) on the handle's stream: a voxel's bit is set iff
        some voxel within inflate_voxels (Chebyshev, 0 .. 8) has mass > threshold.  Read-only towards the map; the grid is a snapshot and
        goes stale with the next frame."""
        self._chk(self.L.dspmap_build_cast_grid(self.h, float(threshold), int(inflate_voxels), 0))

    def cast_grid(self, layer=None):
        """the grid of one layer as numpy uint64 [nz, ny, W], W = ceil(nx / 64), bit (x & 63) of word (x >> 6) = voxel x of the row; or
        of all layers [L, nz, ny, W] (synchronous host copies)"""
        return self._layers("dspmap_get_cast_grid", layer, self.T + 1, (self.cfg.nz, self.cfg.ny, (self.cfg.nx + 63) // 64), np.uint64)

    def cast_grid_ptr(self):
        """device address of the [L][nz][ny][W] uint64 grid, or None when there is none / it is stale"""
        return self.L.dspmap_cast_grid_device(self.h) or None

    def cast_segments(self, seg, world=False):
        """first blocked cell of every segment {ax, ay, az, ta, bx, by, bz, tb} of seg ([n, 8] float32) through the cast grid: the cell
        entered at parameter s is tested in the layer of the time ta + s (tb - ta) (ta < 0: the current layer).  numpy in ->
        structured numpy (HIT_DTYPE: s, voxel, layer, status = CAST_*) out, synchronous; a torch tensor on the GPU -> dict of tensors
        's' (float32), 'voxel', 'layer', 'status' (int32) on the same device, enqueued on the handle's stream and ordered with torch's
        current stream like query_occupancy."""
        q, n, dev = self._input(seg, 8, "cast_segments", "segments of shape [n, 8]")
        out = self._alloc(dev, n, HIT_DTYPE)
        self._call(dev, "dspmap_cast_segments", n, self._p(q), QUERY_WORLD if world else 0, self._p(out))
        return self._fields(out, HIT_DTYPE, dev)

    # -- free boxes in the cast grid (extension; semantics in include/dspmap.h next to dspmap_grow_boxes)
    def grow_boxes(self, seeds, max_grow, world=False, with_current=False):
        """the axis-aligned box of free voxels grown around every seed {ax, ay, az, ta, bx, by, bz, tb} of seeds ([n, 8] float32, the
        segments cast_segments takes) in the cast grid: at most max_grow = (gx, gy, gz) voxels (0 .. 64 each) beyond the seed's own cells
        per side, tested in the layers of the times ta .. tb (ta < 0: the current layer; with_current adds it to the others).  numpy in ->
        structured numpy (BOX_DTYPE: lo[3], hi[3] inclusive voxel indices, status = BOX_*, stop = 2 bits BOX_STOP_* per face) out,
        synchronous; a torch tensor on the GPU -> dict of tensors 'lo', 'hi' ([n, 3] int32), 'status', 'stop' (int32) on the same device,
        enqueued on the handle's stream and ordered with torch's current stream like query_occupancy."""
        flags = (QUERY_WORLD if world else 0) | (BOX_WITH_CURRENT if with_current else 0)
        g = (C.c_int * 3)(*[int(v) for v in max_grow])
        q, n, dev = self._input(seeds, 8, "grow_boxes", "seeds of shape [n, 8]")
        out = self._alloc(dev, n, BOX_DTYPE)
        self._call(dev, "dspmap_grow_boxes", n, self._p(q), C.cast(g, C.c_void_p), flags, self._p(out))
        return self._fields(out, BOX_DTYPE, dev)

    def box_bounds(self, boxes):
        """metric corners (lo_m, hi_m), float32 [n, 3] each, of boxes (BOX_DTYPE, or the dict grow_boxes returns for device input) in the
        map frame: lo_m = fl(fl((float)lo * res) + (-half)), hi_m = fl(fl((float)(hi + 1) * res) + (-half)) per axis, the faces of the
        voxels lo and hi that bound the box; NaN for boxes without indices (BOX_SEED_OUTSIDE, BOX_INVALID).  Host arithmetic."""
        if isinstance(boxes, dict):
            lo, hi = (np.asarray(boxes[k].cpu().numpy() if hasattr(boxes[k], "cpu") else boxes[k], np.int64) for k in ("lo", "hi"))
        else:
            lo, hi = np.asarray(boxes["lo"], np.int64), np.asarray(boxes["hi"], np.int64)
        f = np.float32
        res = f(self.cfg.voxel_resolution)
        half = np.array([f(f(res * f(k)) * f(0.5)) for k in (self.cfg.nx, self.cfg.ny, self.cfg.nz)], f)   # (res * n) * 0.5 (:528-530)
        lo_m = ((lo.astype(f) * res).astype(f) + (-half)).astype(f)
        hi_m = (((hi + 1).astype(f) * res).astype(f) + (-half)).astype(f)
        none = (lo < 0).any(-1)
        lo_m[none], hi_m[none] = np.nan, np.nan
        return lo_m, hi_m

    # -- arrival-time fields (extension; semantics in include/dspmap.h next to dspmap_build_reach_fields)
    @staticmethod
    def _reach_points(pts, what):
        """host points as REACH_POINT_DTYPE [n]: a structured array, or [n, 4] numbers {x, y, z, field}"""
        a = np.asarray(pts)
        if a.dtype == REACH_POINT_DTYPE:
            return np.ascontiguousarray(a).reshape(-1)
        if a.shape[-1:] != (4,):
            raise ValueError("%s: points of shape [n, 4] or of REACH_POINT_DTYPE" % what)
        out = np.zeros(a.size // 4, REACH_POINT_DTYPE)
        a = a.reshape(-1, 4)
        out["x"], out["y"], out["z"] = a[:, 0], a[:, 1], a[:, 2]
        out["field"] = a[:, 3].astype(np.int64)
        return out

    @staticmethod
    def _reach_points_device(pts, what):
        """device points: an int32 or float32 tensor [n, 4] whose last column holds the BITS of the int field (REACH_POINT_DTYPE rows)"""
        import torch
        if pts.dtype not in (torch.float32, torch.int32) or tuple(pts.shape[-1:]) != (4,):
            raise ValueError("%s: a float32 / int32 tensor of shape [n, 4] holding dspmap_reach_point rows" % what)
        return pts.contiguous()

    def build_reach_fields(self, sources, n_fields=1, t_start=-1.0, step_seconds=0.0, max_steps=REACH_MAX_STEPS, world=False,
                           with_current=False, device_sets=False):
        """grow n_fields arrival fields through the cast grid from sources {x, y, z, field}: step n happens at t_start + n * step_seconds
        and tests the grid layer of that time (t_start < 0: the current layer; with_current adds it to the others); a cell's value is
        the first step n <= max_steps at which the 6-connected front holds it.  numpy sources (REACH_POINT_DTYPE, or [n, 4] numbers)
        -> synchronous; a torch tensor on the GPU ([n, 4] int32 / float32 holding the struct's bits) -> enqueued on the handle's stream
        and ordered with torch's current stream like query_occupancy.  Read the result with reach_field / reach_fields_ptr."""
        self._build_reach(False, sources, n_fields, t_start, step_seconds, max_steps, world, with_current, device_sets)

    def _build_reach(self, timeline, sources, n_fields, t_start, step_seconds, max_steps, world, with_current, device_sets):
        """build_reach_fields (timeline False) / build_reach_timeline (True): the same argument list on either pair of entry points"""
        flags = (QUERY_WORLD if world else 0) | (REACH_WITH_CURRENT if with_current else 0) | (REACH_DEVICE_SETS if device_sets else 0)
        q, n, dev = self._input(sources, 4, "build_reach_fields")
        self._call(dev, "dspmap_build_reach_timeline" if timeline else "dspmap_build_reach_fields", int(n_fields), n,
                   self._p(q, n > 0 or dev is not None), float(t_start), float(step_seconds), int(max_steps), flags)

    def reach_field(self, field=None, n_fields=None):
        """the values of one field of the last build as numpy uint16 [nz, ny, nx] (REACH_UNREACHED where the front never came), or with
        field=None those of the first n_fields fields [n_fields, nz, ny, nx] (synchronous host copies)"""
        if field is None and n_fields is None:
            raise ValueError("reach_field: a field, or n_fields for all of them")
        return self._layers("dspmap_get_reach_field", field, n_fields, (self.cfg.nz, self.cfg.ny, self.cfg.nx), np.uint16)

    def reach_fields_ptr(self):
        """device address of the [n_fields][V] uint16 values, or None when there are none / they are stale"""
        return self.L.dspmap_reach_fields_device(self.h) or None

    def reach_storage(self):
        """(fields of the last build whose wave sets lived in LDS, ... in device memory)"""
        return self._counts("dspmap_debug_reach_storage", 2)

    def reach_paths(self, starts, max_len, world=False):
        """descend a time-invariant build from starts {x, y, z, field}: (steps [n] int32: the start's value, -1 unreached, -2 outside the
        map, -3 invalid; cells [n, max_len] int32: voxel indices from the start's cell to a cell of value 0, -1 behind the end).  numpy in
        -> numpy out, synchronous; a torch tensor on the GPU -> tensors on the same device, enqueued like build_reach_fields."""
        return self._paths("dspmap_reach_paths", starts, max_len, world)

    # -- space-time paths (extension; semantics in include/dspmap.h next to dspmap_build_reach_timeline)
    def build_reach_timeline(self, sources, n_fields=1, t_start=-1.0, step_seconds=0.0, max_steps=REACH_MAX_STEPS, world=False,
                             with_current=False, device_sets=False):
        """build_reach_fields -- the same arguments, the same fields, numpy synchronous and a torch GPU tensor enqueued -- that also keeps
        the reached set of every step (n_fields * (max_steps + 1) * nz * ny * W * 8 bytes, at most REACH_TIMELINE_MAX_BYTES): what
        reach_sets hands out and reach_timeline_paths walks backwards through, also where the tested layer changed during the steps."""
        self._build_reach(True, sources, n_fields, t_start, step_seconds, max_steps, world, with_current, device_sets)
        self._timeline_steps = int(max_steps)

    def reach_last_steps(self, n_fields):
        """int32 [n_fields]: the last step each field of the last timeline build executed (a later step repeats its set); synchronous"""
        out = np.zeros(REACH_MAX_FIELDS, np.int32)
        self._chk(self.L.dspmap_reach_last_steps(self.h, _ptr(out)))
        return out[:int(n_fields)].copy()

    def reach_sets(self, field, first_step=0, n_steps=None):
        """the sets R_first_step .. of one field of the last timeline build as numpy uint64 [n_steps, nz, ny, W] (bit x & 63 of word
        x >> 6, as cast_grid); n_steps=None: every step from first_step to the build's max_steps.  Steps behind the field's last executed
        one repeat it.  Synchronous host copy."""
        n = max(getattr(self, "_timeline_steps", 0) + 1 - int(first_step), 0) if n_steps is None else int(n_steps)
        out = np.zeros((max(n, 0), self.cfg.nz, self.cfg.ny, (self.cfg.nx + 63) // 64), np.uint64)
        self._chk(self.L.dspmap_get_reach_sets(self.h, int(field), int(first_step), n, _ptr(out) if n > 0 else None))
        return out

    def reach_timeline_ptr(self):
        """device address of the rows [n_fields][max_steps + 1][nz][ny][W], or None when there are none / they are stale"""
        return self.L.dspmap_reach_timeline_device(self.h) or None

    def reach_timeline_paths(self, starts, max_len, world=False):
        """walk backwards through the sets of the last timeline build from starts {x, y, z, field}: (steps [n] int32: the start's first
        arrival v, -1 unreached, -2 outside the map, -3 invalid; cells [n, max_len] int32: the voxel occupied at step v - j, waits
        included, down to a source cell at step 0, -1 behind the end).  numpy in -> numpy out, synchronous; a torch tensor on the GPU ->
        tensors on the same device, enqueued like reach_paths."""
        return self._paths("dspmap_reach_timeline_paths", starts, max_len, world)

    # -- cost-to-go fields (extension; semantics in include/dspmap.h next to dspmap_build_cost_fields)
    @staticmethod
    def _cost_bands(bands):
        """a sequence of (clearance, penalty) as dspmap_cost_bands; more than COST_MAX_BANDS of them keep their count, for the library to refuse"""
        bands = list(bands)
        b = CostBands()
        b.n_bands = len(bands)
        for i, (clearance, penalty) in enumerate(bands[:COST_MAX_BANDS]):
            b.clearance[i], b.penalty[i] = float(clearance), int(penalty)
        return b

    def build_cost_fields(self, sources, n_fields=1, t=-1.0, bands=(), max_cost=COST_MAX_COST, world=False):
        """grow n_fields cost-to-go fields from sources {x, y, z, field} through ONE layer of the cast grid (t < 0: the current one, else
        the horizon of t): entering a free cell costs 1 plus the penalty of every band (clearance, penalty) whose clearance the cell's
        value in the distance field lies under; a cell's value is its exact minimum cost if <= max_cost, else COST_UNREACHED.  Needs the
        cast grid and, with bands, the distance field.  numpy sources -> synchronous; a torch tensor on the GPU -> enqueued like
        build_reach_fields.  Read the result with cost_field / cost_fields_ptr / cost_weights, descend it with cost_paths."""
        b = self._cost_bands(bands)
        q, n, dev = self._input(sources, 4, "build_cost_fields")
        self._call(dev, "dspmap_build_cost_fields", int(n_fields), n, self._p(q, n > 0 or dev is not None), float(t), C.addressof(b), int(max_cost),
                   QUERY_WORLD if world else 0)

    def cost_field(self, field=None, n_fields=None):
        """the values of one field of the last cost build as numpy uint16 [nz, ny, nx] (COST_UNREACHED where the cost exceeds max_cost or
        no path exists), or with field=None those of the first n_fields fields [n_fields, nz, ny, nx] (synchronous host copies)"""
        if field is None and n_fields is None:
            raise ValueError("cost_field: a field, or n_fields for all of them")
        return self._layers("dspmap_get_cost_field", field, n_fields, (self.cfg.nz, self.cfg.ny, self.cfg.nx), np.uint16)

    def cost_fields_ptr(self):
        """device address of the [n_fields][V] uint16 values, or None when there are none / they are stale"""
        return self.L.dspmap_cost_fields_device(self.h) or None

    def cost_weights(self):
        """the weights of the last cost build as numpy uint8 [nz, ny, nx]: 0 blocked, else what entering the cell costs"""
        out = np.zeros((self.cfg.nz, self.cfg.ny, self.cfg.nx), np.uint8)
        self._chk(self.L.dspmap_get_cost_weights(self.h, _ptr(out)))
        return out

    def cost_paths(self, starts, max_len, world=False):
        """descend the last cost build from starts {x, y, z, field}: (cost [n] int32: the start's value, -1 unreached, -2 outside the
        map, -3 invalid; cells [n, max_len] int32: voxel indices from the start's cell to a cell of value 0, -1 behind the end) -- what
        shorten_paths takes as (steps, cells).  numpy in -> numpy out, synchronous; a torch tensor on the GPU -> tensors on the same
        device, enqueued like build_cost_fields."""
        return self._paths("dspmap_cost_paths", starts, max_len, world)

    # -- shortened paths (extension; semantics in include/dspmap.h next to dspmap_shorten_paths)
    def shorten_paths(self, steps, cells, t_start=-1.0, step_seconds=0.0, window=SHORTEN_MAX_WINDOW, max_seg=None):
        """cut cell paths (steps [n] int32, cells [n, max_len] int32: what reach_paths and reach_timeline_paths return, or any polyline
        of voxel indices ended by -1) down to line-of-sight waypoints in the cast grid: from each anchor the farthest of the next `window`
        (1 .. 64) cells that cast_segments calls free, the next cell where none is.  With the t_start and step_seconds of the build the
        paths came from, cell j gets the time of the step it is occupied at (t_start < 0: the current layer).  Returns (info, segments,
        ends): info PATH_INFO_DTYPE [n] (n_cells, n_segments, n_blocked, truncated), segments float32 [n, max_seg, 8] -- the records
        cast_segments and grow_boxes take, all zero behind n_segments -- and ends int32 [n, max_seg], the path position each segment ends
        at (-1 behind n_segments).  max_seg=None: max_len - 1, which never truncates.  numpy in -> numpy out, synchronous; torch tensors
        on the GPU -> tensors on the same device (info as int32 [n, 4]), enqueued on the handle's stream and ordered with torch's current
        stream like cast_segments."""
        if self._is_device_tensor(cells):
            import torch
            if cells.dtype != torch.int32 or cells.dim() != 2 or not self._is_device_tensor(steps) or steps.dtype != torch.int32 or \
                    steps.device != cells.device or steps.numel() != cells.shape[0]:
                raise ValueError("shorten_paths: int32 tensors steps [n] and cells [n, max_len] on one device")
            c, s, dev = cells.contiguous(), steps.contiguous().view(-1), cells.device
        else:
            c, s, dev = np.ascontiguousarray(cells, np.int32), np.ascontiguousarray(steps, np.int32).reshape(-1), None
            if c.ndim != 2 or len(s) != c.shape[0]:
                raise ValueError("shorten_paths: steps [n] and cells [n, max_len]")
        n, max_len = int(c.shape[0]), int(c.shape[1])
        ms = max(max_len - 1, 0) if max_seg is None else int(max_seg)
        info = self._alloc(dev, n, PATH_INFO_DTYPE)
        seg = self._alloc(dev, (n, max(ms, 0), 8), np.float32)
        end = self._alloc(dev, (n, max(ms, 0)), np.int32)
        self._call(dev, "dspmap_shorten_paths", n, max_len, self._p(s, n), self._p(c, n), float(t_start), float(step_seconds), int(window), ms, 0,
                   self._p(info, n), self._p(seg, n and ms > 0), self._p(end, n and ms > 0))
        return info, seg, end

    # -- occupancy forecast at caller-chosen times (extension; semantics in include/dspmap.h next to dspmap_build_forecast)
    def build_forecast(self, times):
        """enqueue the occupancy layers at `times` (seconds after the last frame: strictly ascending, finite, >= 0, at most
        FORECAST_MAX_TIMES of them) on the handle's stream: every live particle rolled out to each time, newborns included, no weight
        cull.  Read-only towards the map; the layers are a snapshot and go stale with the next frame."""
        t = np.ascontiguousarray(times, np.float32).reshape(-1)
        self._chk(self.L.dspmap_build_forecast(self.h, len(t), _ptr(t) if len(t) else None, 0))

    def forecast_times(self):
        """the times of the valid snapshot, float32 [n]"""
        t = np.zeros(FORECAST_MAX_TIMES, np.float32)
        n = self.L.dspmap_forecast_times(self.h, _ptr(t), len(t))
        if n < 0:
            self._chk(n)
        return t[:n].copy()

    def forecast(self, layer=None):
        """one layer as numpy [V] (the reference's voxel order), or all layers [n, V] (synchronous host copies)"""
        V = self.L.dspmap_voxel_num(self.h)
        return self._layers("dspmap_get_forecast", layer, len(self.forecast_times()) if layer is None else 0, (V,), np.float32)

    def forecast_ptr(self):
        """device address of the [n][V] float32 layers, or None when there are none / they are stale"""
        return self.L.dspmap_forecast_device(self.h) or None

    def query_forecast(self, q, world=False, lerp=False, outside=1.0):
        """value of every sample {x, y, z, t} of q ([n, 4] float32) at its own voxel: the first layer whose time is >= t (the last one
        beyond it), or with lerp the fp32 interpolation between that layer and the one before; `outside` for what lies outside the map.
        numpy in -> numpy out (synchronous); a torch tensor on the GPU -> a tensor on the same device, enqueued on the handle's stream
        and ordered with torch's current stream like query_occupancy."""
        flags = (QUERY_WORLD if world else 0) | (FORECAST_LERP if lerp else 0)
        return self._query("dspmap_query_forecast", q, np.float32, (flags, float(outside)))

    # -- known-space layer (extension; semantics in include/dspmap.h next to dspmap_known_integrate)
    def integrate_known(self, max_range=float("inf")):
        """enqueue the integration of the last frame's view into the known-space layer on the handle's stream: every world lattice cell
        of the window whose centre lies in a pyramid of the frame, not behind that pyramid's farthest return (plus the occlusion margin)
        and within max_range of the sensor is stamped with the update counter.  Read-only towards the map."""
        self._chk(self.L.dspmap_known_integrate(self.h, float(max_range), 0))

    def reset_known(self):
        """forget everything the layer has seen"""
        self._chk(self.L.dspmap_known_reset(self.h))

    def known_age(self):
        """frames since each voxel was last seen, -1 = never: numpy int32 [nz, ny, nx] (synchronous host copy)"""
        out = np.zeros((self.cfg.nz, self.cfg.ny, self.cfg.nx), np.int32)
        self._chk(self.L.dspmap_get_known(self.h, _ptr(out)))
        return out

    def query_known(self, q, world=False):
        """age of the cell that holds every sample {x, y, z, t} of q ([n, 4] float32; t is ignored), -1 outside the map, for a NaN
        coordinate or for a cell never seen.  numpy in -> numpy int32 out (synchronous); a torch tensor on the GPU -> an int32 tensor on
        the same device, enqueued on the handle's stream and ordered with torch's current stream like query_occupancy."""
        return self._query("dspmap_query_known", q, np.int32, (QUERY_WORLD if world else 0,), init_device=True)

    def mask_cast_grid(self, max_age):
        """OR "unknown" into every layer of the valid cast grid: the bit of each voxel never seen or seen more than max_age frames ago.
        Casts, boxes and arrival fields built afterwards treat that space as blocked; arrival fields built before are stale."""
        self._chk(self.L.dspmap_mask_cast_grid(self.h, int(max_age), 0))

    def known_stats(self, max_age):
        """(cells with 0 <= age <= max_age, cells stamped by the current frame)"""
        return self._counts("dspmap_known_stats", 2, int(max_age))

    def view(self):
        """(planes_h [np_h + 1, 3], planes_v [np_v + 1, 3], maxlen [np_h, np_v]) of the last frame: the rotated boundary-plane normals and
        the farthest return per pyramid (-1 = none), float32 host copies (synchronous)"""
        nh = 2 * self.cfg.half_fov_h // self.cfg.angle_resolution
        nv = 2 * self.cfg.half_fov_v // self.cfg.angle_resolution
        assert nh * nv == self.NP
        ph, pv, ml = np.zeros((nh + 1, 3), np.float32), np.zeros((nv + 1, 3), np.float32), np.zeros((nh, nv), np.float32)
        self._chk(self.L.dspmap_get_view(self.h, _ptr(ph), _ptr(pv), _ptr(ml)))
        return ph, pv, ml

    # -- scores of candidate viewpoints (extension; semantics in include/dspmap.h next to dspmap_score_views)
    def score_views(self, views, max_age, world=False):
        """what a frame taken from every view {x, y, z, qw, qx, qy, qz, max_range, t} of views ([n, 9] float32) would see in the cast grid
        as it is: the voxels in its wedge, not behind the first blocked cell of their pyramid's central ray and within max_range
        (n_seen), those of them whose age in the known-space layer is -1 or > max_age (n_unknown), and the rays that hit (n_returns).
        numpy in -> structured numpy (VIEW_SCORE_DTYPE, status = VIEW_*) out, synchronous; a torch tensor on the GPU -> an int32 [n, 4]
        tensor {n_seen, n_unknown, n_returns, status} on the same device, enqueued on the handle's stream and ordered with torch's
        current stream like query_known."""
        q, n, dev = self._input(views, 9, "score_views", "views of shape [n, 9]")
        out = self._alloc(dev, n, VIEW_SCORE_DTYPE)
        self._call(dev, "dspmap_score_views", n, self._p(q), int(max_age), QUERY_WORLD if world else 0, self._p(out))
        return out

    # -- joint gain of views (extension; semantics in include/dspmap.h next to dspmap_score_view_sets)
    def score_view_sets(self, views, max_age, world=False, scores=False):
        """what every SET of views sees together: views [n_sets, set_size, 9] float32 -> per set the voxels in the union of the members'
        seen sets (n_seen), those of them that are unknown (n_unknown) and the members whose status is VIEW_OK (n_ok); a short set is
        padded with views whose max_range is 0.  scores=True: also every view's score_views score.  numpy in -> structured numpy
        (VIEW_SET_SCORE_DTYPE [n_sets], and VIEW_SCORE_DTYPE [n_sets, set_size]) out, synchronous; a torch tensor on the GPU -> int32
        tensors [n_sets, 4] (and [n_sets, set_size, 4]) on the same device, enqueued on the handle's stream and ordered with torch's
        current stream like score_views."""
        q, _, dev = self._input(views, 9, "score_view_sets", "views of shape [n_sets, set_size, 9]", ndim=3)
        ns, sz = int(q.shape[0]), int(q.shape[1])
        out = self._alloc(dev, ns, VIEW_SET_SCORE_DTYPE)
        sc = self._alloc(dev, (ns, sz), VIEW_SCORE_DTYPE) if scores else None
        self._call(dev, "dspmap_score_view_sets", ns, sz, self._p(q), int(max_age), QUERY_WORLD if world else 0, self._p(out), self._p(sc))
        return (out, sc) if scores else out

    def select_views(self, views, k, max_age, n_fixed=0, min_gain=1, world=False, scores=False):
        """the greedy choice of k of the views [n, 9] float32 that see the most unknown space TOGETHER: views [0, n_fixed) are committed
        already, every round picks the candidate of [n_fixed, n) that adds the most unknown voxels to what is covered (the smallest
        index among equals) until a round's best adds fewer than min_gain; VIEW_PICK_DTYPE [k] {view, gain, covered}, view = -1 from
        the first empty round on.  scores=True: also every view's score_views score [n].  numpy in -> structured numpy out,
        synchronous; a torch tensor on the GPU -> int32 tensors [k, 4] (and [n, 4]) on the same device, every round enqueued on the
        handle's stream without a host read in between, ordered with torch's current stream like score_views."""
        q, n, dev = self._input(views, 9, "select_views", "views of shape [n, 9]", ndim=2)
        out = self._alloc(dev, max(int(k), 0), VIEW_PICK_DTYPE)
        sc = self._alloc(dev, n, VIEW_SCORE_DTYPE) if scores else None
        self._call(dev, "dspmap_select_views", n, self._p(q), int(n_fixed), int(max_age), QUERY_WORLD if world else 0, int(k), int(min_gain),
                   self._p(out), self._p(sc))
        return (out, sc) if scores else out

    def view_rays(self, quat):
        """(planes_h [np_h + 1, 3], planes_v [np_v + 1, 3], dirs [NP, 3]) of an attitude (w, x, y, z): the rotated boundary-plane normals a
        frame with that attitude has, and the central ray of every pyramid, float32 host copies made on the device (synchronous)"""
        nh = 2 * self.cfg.half_fov_h // self.cfg.angle_resolution
        nv = 2 * self.cfg.half_fov_v // self.cfg.angle_resolution
        q = np.ascontiguousarray(quat, np.float32)
        if q.shape != (4,):
            raise ValueError("view_rays: a quaternion (w, x, y, z)")
        ph, pv, dirs = np.zeros((nh + 1, 3), np.float32), np.zeros((nv + 1, 3), np.float32), np.zeros((nh * nv, 3), np.float32)
        self._chk(self.L.dspmap_view_rays(self.h, _ptr(q), _ptr(ph), _ptr(pv), _ptr(dirs)))
        return ph, pv, dirs

    def view_cells(self, view, world=False):
        """test hook: (seen [nz, ny, W] uint64 in the cast grid's word layout, ml [NP] float32) of ONE view ([9] float32): the cells
        score_views counts in n_seen and the farthest return every pyramid's ray gave (-1 = none); synchronous"""
        q = np.ascontiguousarray(view, np.float32)
        if q.shape != (9,):
            raise ValueError("view_cells: one view of shape [9]")
        words = np.zeros((self.cfg.nz, self.cfg.ny, (self.cfg.nx + 63) // 64), np.uint64)
        ml = np.zeros(self.NP, np.float32)
        self._chk(self.L.dspmap_debug_view_cells(self.h, _ptr(q), QUERY_WORLD if world else 0, _ptr(words), _ptr(ml)))
        return words, ml

    # -- frontier cells and blocks (extension; semantics in include/dspmap.h next to dspmap_build_frontiers)
    def build_frontiers(self, t=-1.0, max_age=0, min_unknown=1, block=4):
        """enqueue the frontier of the layer t selects of the cast grid as it is, on the handle's stream: the cells that are known (0 <=
        age <= max_age) with a clear bit and at least min_unknown (1 .. 6) of whose face neighbours inside the map are unknown, as a bit
        grid, as an ascending list of voxel indices and summed over blocks of block^3 voxels (1 .. 32).  Read-only towards the map, the
        grid and the layer; the result is a snapshot of all three."""
        self._chk(self.L.dspmap_build_frontiers(self.h, float(t), int(max_age), int(min_unknown), int(block), 0))

    def frontier_counts(self):
        """(n_cells, n_blocks, n_free) of the last build (synchronous)"""
        return self._counts("dspmap_frontier_counts", 3)

    def frontier_grid(self):
        """the frontier bits as numpy uint64 [nz, ny, W] in the cast grid's word layout (synchronous host copy)"""
        out = np.zeros((self.cfg.nz, self.cfg.ny, (self.cfg.nx + 63) // 64), np.uint64)
        self._chk(self.L.dspmap_get_frontier_grid(self.h, _ptr(out)))
        return out

    def frontier_cells(self, device=None):
        """the voxel indices of the frontier cells in ascending order: numpy int32 [n] (synchronous host copy); with device= (e.g. "cuda")
        an int32 tensor [n] over the handle's own device buffer, without a copy, ordered with torch's current stream like score_views.
        The tensor is valid until the next build_frontiers or close()."""
        if device is not None:   # (the count is read from the device, which synchronises the handle's stream and raises on a stale snapshot)
            return self._span(device, "dspmap_frontier_cells_device", (self.frontier_counts()[0],))
        return self._list("dspmap_get_frontier_cells", np.dtype(np.int32))

    def frontier_blocks(self, device=None):
        """the records of the non-empty blocks in ascending block index: structured numpy (FRONTIER_BLOCK_DTYPE) [k] (synchronous host
        copy); with device= an int32 tensor [k, 6] {block, count, sum_x, sum_y, sum_z, unknown_faces} over the handle's own device
        buffer, without a copy, as frontier_cells"""
        if device is not None:
            return self._span(device, "dspmap_frontier_blocks_device", (self.frontier_counts()[1], 6))
        return self._list("dspmap_get_frontier_blocks", FRONTIER_BLOCK_DTYPE)

    def frontier_block_centers(self, min_count=1):
        """float32 [k, 3]: the centroid of the frontier cells of every block with at least min_count of them, in the map frame:
        ((sum / count) + 0.5) * res - half per axis (a mean voxel index is the centre of that voxel)"""
        b = self.frontier_blocks()
        b = b[b["count"] >= int(min_count)]
        cfg = self.cfg
        res = float(np.float32(cfg.voxel_resolution))
        half = np.array([cfg.nx, cfg.ny, cfg.nz], np.float64) * res / 2.0
        mean = np.stack([b["sum_x"], b["sum_y"], b["sum_z"]], 1) / np.maximum(b["count"], 1)[:, None]
        return ((mean + 0.5) * res - half).astype(np.float32)

    # -- objects: components of a cast-grid layer (extension; semantics in include/dspmap.h next to dspmap_build_objects)
    def build_objects(self, t=-1.0, connectivity=26, min_cells=1, max_objects=4096):
        """enqueue the labelling of the layer t selects of the cast grid as it is, on the handle's stream: its connected components under
        6- or 26-connectivity, those with at least min_cells cells as records (box, index sums, fixed-point mass and momentum from the
        current result grid) in ascending label, the first max_objects kept, and a label grid.  Read-only towards the map and the grid;
        the result is a snapshot of both."""
        self._chk(self.L.dspmap_build_objects(self.h, float(t), int(connectivity), int(min_cells), int(max_objects), 0))

    def object_counts(self):
        """(n_objects, n_components, n_occupied) of the last build (synchronous): components with count >= min_cells -- also those past
        max_objects --, all components, set bits of the layer"""
        return self._counts("dspmap_object_counts", 3)

    def objects(self, device=None):
        """the records the last build kept, in ascending label: structured numpy (OBJECT_DTYPE) [k], k = min(n_objects, max_objects)
        (synchronous host copy); with device= (e.g. "cuda") an int32 tensor [k, 22] over the handle's own device buffer, without a copy
        -- columns 0 .. 7 the ints, then the seven 64-bit fields as (low, high) pairs; `t[:, 8:].view(torch.int64)` gives them as [k, 7] --,
        ordered with torch's current stream like frontier_cells and valid until the next build_objects or close()."""
        return self._list("dspmap_get_objects", OBJECT_DTYPE, device, "dspmap_objects_device")

    def object_labels(self, device=None):
        """the label grid of the last build: numpy int32 [nz, ny, nx], per voxel the ordinal of its record in the list of objects (also an
        ordinal >= max_objects), -1 for a clear bit or a component below min_cells (synchronous host copy); with device= an int32 tensor
        of that shape over the handle's own device buffer, without a copy, as objects()"""
        shape = (self.cfg.nz, self.cfg.ny, self.cfg.nx)
        if device is not None:
            self.object_counts()   # (synchronises the handle's stream; raises on a stale snapshot)
            return self._span(device, "dspmap_object_labels_device", shape)
        out = np.zeros(shape, np.int32)
        self._chk(self.L.dspmap_get_object_labels(self.h, _ptr(out)))
        return out

    def query_objects(self, q, world=False):
        """the label-grid entry of the voxel that holds every sample {x, y, z, t} of q ([n, 4] float32; t is ignored), -1 outside the map
        or for a NaN coordinate.  numpy in -> numpy int32 out (synchronous); a torch tensor on the GPU -> an int32 tensor on the same
        device, enqueued on the handle's stream and ordered with torch's current stream like query_known."""
        return self._query("dspmap_query_objects", q, np.int32, (QUERY_WORLD if world else 0,))

    def object_states(self, objs):
        """what a planner takes from the records objs (OBJECT_DTYPE, what objects() returns), in the map frame: (centre [k, 3], box_lo
        [k, 3], box_hi [k, 3], velocity [k, 3]), float32.  centre = the mean voxel index as a position, ((sum / count) + 0.5) * res -
        half per axis (dspmap_voxel_center's expression on a mean index); box_lo / box_hi = the outer corners of the voxels min / max;
        velocity = mom_q / mass_q in m/s, 0 where the object holds no mass."""
        cfg = self.cfg
        res = float(np.float32(cfg.voxel_resolution))
        half = np.array([cfg.nx, cfg.ny, cfg.nz], np.float64) * res / 2.0
        cnt = np.maximum(objs["count"], 1)[:, None].astype(np.float64)
        mean = np.stack([objs["sum_x"], objs["sum_y"], objs["sum_z"]], 1) / cnt
        lo = np.stack([objs["min_x"], objs["min_y"], objs["min_z"]], 1).astype(np.float64)
        hi = np.stack([objs["max_x"], objs["max_y"], objs["max_z"]], 1).astype(np.float64)
        mass = objs["mass_q"].astype(np.float64)[:, None]
        vel = np.where(mass > 0, objs["mom_q"].astype(np.float64) / np.maximum(mass, 1.0), 0.0)
        return (((mean + 0.5) * res - half).astype(np.float32), (lo * res - half).astype(np.float32),
                ((hi + 1.0) * res - half).astype(np.float32), vel.astype(np.float32))

    # -- tracks: objects across builds (extension; semantics in include/dspmap.h next to dspmap_track_update)
    def update_tracks(self, dt, min_overlap=1, max_shift=8, max_pairs=0, per_cell=False):
        """enqueue the association of the objects of the valid build_objects with those the previous update_tracks saw, on the handle's
        stream: voxel overlap after each previous object's predicted shift (velocity * dt, at most max_shift voxels, and the window's
        move), mutual best matches with at least min_overlap cells.  A matched object inherits its id, an unmatched one gets a fresh
        id; tracks()[i] belongs to objects()[i].  max_pairs: slots of the pair table (0: 8 x the record capacity); per_cell: one table
        insert per cell instead of one per run, the same result."""
        self._chk(self.L.dspmap_track_update(self.h, float(dt), int(min_overlap), int(max_shift), int(max_pairs), TRACK_PER_CELL if per_cell else 0))

    def reset_tracks(self):
        """forget every track and the stored previous objects; ids start at 0 again"""
        self._chk(self.L.dspmap_track_reset(self.h))

    def track_counts(self):
        """(n_tracks, n_matched, n_born, n_ended, n_pairs, next_id) of the last update (synchronous)"""
        return self._counts("dspmap_track_counts", 6)

    def tracks(self, device=None):
        """the tracks of the last update, one per record of objects(): structured numpy (TRACK_DTYPE) [k] (synchronous host copy); with
        device= (e.g. "cuda") an int32 tensor [k, 18] over the handle's own device buffer, without a copy -- columns 0 .. 9 the five
        64-bit fields as (low, high) pairs, `t[:, :10].view(torch.int64)` gives them as [k, 5], then the eight ints --, ordered with
        torch's current stream like objects() and valid until the next update_tracks, reset_tracks or close()."""
        return self._list("dspmap_get_tracks", TRACK_DTYPE, device, "dspmap_tracks_device")

    def track_states(self, tracks, objs, dt):
        """what a planner takes from the tracks (TRACK_DTYPE) and their records objs (OBJECT_DTYPE) of the same update: (displacement
        [k, 3], velocity [k, 3]), float32 -- the centroid's displacement since the previous update in metres, (sum / count - prev_sum /
        prev_count) * res per axis, and the velocity measured from it, displacement / dt (0 for dt <= 0); both 0 for a born track."""
        res = float(np.float32(self.cfg.voxel_resolution))
        cnt = np.maximum(objs["count"], 1)[:, None].astype(np.float64)
        pcnt = np.maximum(tracks["prev_count"], 1)[:, None].astype(np.float64)
        mean = np.stack([objs["sum_x"], objs["sum_y"], objs["sum_z"]], 1) / cnt
        prev = np.stack([tracks["prev_sum_x"], tracks["prev_sum_y"], tracks["prev_sum_z"]], 1) / pcnt
        disp = np.where((tracks["prev_ordinal"] >= 0)[:, None], (mean - prev) * res, 0.0)
        vel = disp / float(dt) if float(dt) > 0.0 else np.zeros_like(disp)
        return disp.astype(np.float32), vel.astype(np.float32)

    def set_known(self, ages):
        """test hook: replace the ages of the known-space layer (int32 [nz, ny, nx], what known_age() returns; -1 = never, else 0 ..
        update counter - 1); the layer counts as integrated"""
        a = np.ascontiguousarray(ages, np.int32)
        shape = (self.cfg.nz, self.cfg.ny, self.cfg.nx)
        if a.shape != shape:
            raise ValueError("set_known: ages of shape %s" % (shape,))
        self._chk(self.L.dspmap_debug_set_known(self.h, _ptr(a)))

    def set_cast_grid(self, words):
        """test hook: replace all layers of the valid cast grid with words (uint64 [L, nz, ny, W], what cast_grid() returns)"""
        w = np.ascontiguousarray(words, np.uint64)
        shape = (self.T + 1, self.cfg.nz, self.cfg.ny, (self.cfg.nx + 63) // 64)
        if w.shape != shape:
            raise ValueError("set_cast_grid: words of shape %s" % (shape,))
        self._chk(self.L.dspmap_debug_set_cast_grid(self.h, _ptr(w)))

    def set_distance_field(self, layers):
        """test hook: replace all layers of the valid distance field with layers (float32 [L, nz, ny, nx], what distance_field() returns
        per layer)"""
        a = np.ascontiguousarray(layers, np.float32)
        shape = (self.T + 1, self.cfg.nz, self.cfg.ny, self.cfg.nx)
        if a.shape != shape:
            raise ValueError("set_distance_field: layers of shape %s" % (shape,))
        self._chk(self.L.dspmap_debug_set_distance_field(self.h, _ptr(a)))

    def getVoxelPositionFromIndexPublic(self, index):
        x, y, z = C.c_float(), C.c_float(), C.c_float()
        self.L.dspmap_voxel_center(self.h, index, C.byref(x), C.byref(y), C.byref(z))
        return x.value, y.value, z.value

    def getPointVoxelsIndexPublic(self, px, py, pz):
        idx = C.c_int()
        ok = self.L.dspmap_point_voxel_index(self.h, px, py, pz, C.byref(idx))
        return ok, idx.value

    def debug_tile_fov(self):
        n = self.tile_count()
        out = np.zeros(n, np.int32)
        got = self.L.dspmap_debug_tile_view(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), n)
        if got < 0:
            self._chk(got)
        return out[:got]

    def counters(self):
        c = Counters()
        self._chk(self.L.dspmap_get_counters(self.h, C.byref(c)))
        return c.as_dict()

    STAGES = ("setup+bin", "predict", "claim", "ck_partial", "weight", "ck_finalize", "birth", "resample")

    def set_profiling(self, on=True):
        self._chk(self.L.dspmap_set_profiling(self.h, 1 if on else 0))

    def stage_ms(self):
        """(per-stage summed device ms, frames) accumulated since set_profiling(True)"""
        out = (C.c_float * 8)()
        n = C.c_int()
        self._chk(self.L.dspmap_get_stage_ms(self.h, out, C.byref(n)))
        return dict(zip(self.STAGES, list(out))), n.value

    def event_overhead_ms(self):
        """what an event bracket adds to the one kernel inside it (calibrated by set_profiling(True))"""
        out = C.c_float()
        self._chk(self.L.dspmap_get_event_overhead_ms(self.h, C.byref(out)))
        return out.value

    # -- state
    def clear_state(self):
        self._chk(self.L.dspmap_clear_state(self.h))

    def import_state(self, voxel, rec8, slot=None):
        voxel = np.ascontiguousarray(voxel, np.int32)
        rec8 = np.ascontiguousarray(rec8, np.float32).reshape(-1, 8)
        s = np.ascontiguousarray(slot, np.int32) if slot is not None else None
        self._chk(self.L.dspmap_import_state(self.h, voxel.size, _ptr(voxel), _ptr(s), _ptr(rec8)))

    def export_state(self):
        cap = self.V_local * self.slots
        n = C.c_int()
        self._chk(self.L.dspmap_export_state(self.h, 0, None, None, None, C.byref(n)))
        cap = n.value
        voxel = np.zeros(cap, np.int32)
        slot = np.zeros(cap, np.int32)
        rec = np.zeros((cap, 8), np.float32)
        if cap:
            self._chk(self.L.dspmap_export_state(self.h, cap, _ptr(voxel), _ptr(slot), _ptr(rec), C.byref(n)))
        order = np.lexsort((slot, voxel))
        return voxel[order], slot[order], rec[order]

    def save_checkpoint(self, path):
        self._chk(self.L.dspmap_save_checkpoint(self.h, str(path).encode()))

    def load_checkpoint(self, path):
        self._chk(self.L.dspmap_load_checkpoint(self.h, str(path).encode()))

    def preprocess_cloud(self, points_ptr, n, out_ptr, max_points, leaf=0.1, swap_axes=True, stride=3):
        """voxel-grid filter + axis swap + crop + cap on the device (src/map_sim_example.cpp:309-336);
        returns (points written to out_ptr, occupied leaves touching the map box)"""
        n_out, n_leaves = C.c_int(), C.c_int()
        self._chk(self.L.dspmap_preprocess_cloud(self.h, n, points_ptr, stride, leaf, 1 if swap_axes else 0, max_points,
                                                 out_ptr, C.byref(n_out), C.byref(n_leaves)))
        return n_out.value, n_leaves.value

    # -- depth images (include/dspmap.h next to dspmap_preprocess_depth)
    @staticmethod
    def _host_image(cam, depth):
        """a numpy image laid out as `cam` says: dtype from the format, rows cam.row_stride_bytes apart (0 = packed)"""
        dt = np.uint16 if cam.format == DEPTH_U16 else np.float32
        depth = np.asarray(depth)
        if depth.dtype != dt:
            raise ValueError("depth image: dtype %s for format %d" % (depth.dtype, cam.format))
        if cam.row_stride_bytes == 0:
            depth = np.ascontiguousarray(depth)
            if depth.size != cam.width * cam.height:
                raise ValueError("depth image: %d pixels for a %d x %d camera" % (depth.size, cam.width, cam.height))
        else:
            need = cam.row_stride_bytes * (cam.height - 1) + cam.width * depth.itemsize
            if not depth.flags["C_CONTIGUOUS"] or depth.nbytes < need:
                raise ValueError("depth image: a C-contiguous buffer of at least %d bytes for this row stride" % need)
        return depth

    def _device_image(self, cam, depth):
        import torch
        ok = (torch.int16, getattr(torch, "uint16", torch.int16)) if cam.format == DEPTH_U16 else (torch.float32,)
        if depth.dtype not in ok:
            raise ValueError("depth image: dtype %s for format %d" % (depth.dtype, cam.format))
        depth = depth.contiguous()
        row = cam.row_stride_bytes or cam.width * depth.element_size()
        if depth.numel() * depth.element_size() < row * (cam.height - 1) + cam.width * depth.element_size():
            raise ValueError("depth image: too few bytes for a %d x %d camera" % (cam.width, cam.height))
        return depth

    def preprocess_depth(self, cam, depth, max_points=5000, leaf=0.1):
        """depth image (torch tensor on the GPU: uint16 / int16 bits for DEPTH_U16, float32 for DEPTH_F32) -> (filtered cloud as an
        [n, 3] float32 tensor on the same device, occupied leaves touching the map box, pixels that passed the validity and range
        test).  Back-projection, voxel-grid centroid filter, axis swap, crop and cap in one pass on the device; synchronous."""
        import torch
        if not self._is_device_tensor(depth):
            raise ValueError("preprocess_depth: a torch tensor on the GPU (update_depth takes host images)")
        depth = self._device_image(cam, depth)
        out = torch.empty((max(int(max_points), 0), 3), dtype=torch.float32, device=depth.device)
        n_out, n_leaves, n_valid = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.dspmap_init_device(self.h))
        before, after = self._handle_stream_order(depth.device)
        before()
        self._chk(self.L.dspmap_preprocess_depth(self.h, C.byref(cam), depth.data_ptr(), float(leaf), int(max_points),
                                                 out.data_ptr() if max_points > 0 else None, C.byref(n_out), C.byref(n_leaves),
                                                 C.byref(n_valid)))
        after()
        return out[:n_out.value], n_leaves.value, n_valid.value

    def update_depth(self, cam, depth, pos, stamp, quat, max_points=5000, leaf=0.1):
        """the whole frame from one depth image: a numpy image goes through dspmap_update_depth (one copy of the IMAGE over the bus), a
        torch tensor on the GPU through dspmap_update_depth_device.  Returns 1 (ok) / 0 (rejected)."""
        pos_a = (C.c_float * 3)(*pos)
        q_a = (C.c_float * 4)(*quat)
        if self._is_device_tensor(depth):
            depth = self._device_image(cam, depth)
            self._chk(self.L.dspmap_init_device(self.h))
            before, after = self._handle_stream_order(depth.device)
            before()
            rc = self._chk(self.L.dspmap_update_depth_device(self.h, C.byref(cam), depth.data_ptr(), float(leaf), int(max_points),
                                                             C.cast(pos_a, C.c_void_p), float(stamp), C.cast(q_a, C.c_void_p)))
            after()
            return rc
        depth = self._host_image(cam, depth)
        return self._chk(self.L.dspmap_update_depth(self.h, C.byref(cam), _ptr(depth), float(leaf), int(max_points),
                                                    C.cast(pos_a, C.c_void_p), float(stamp), C.cast(q_a, C.c_void_p)))

    def seed_uniform(self, per_voxel, weight=0.01, seed=99, vmax=0.0):
        self._chk(self.L.dspmap_seed_uniform_moving(self.h, per_voxel, weight, seed, vmax))

    # -- stages
    def bin_points(self, pts, quat=(1, 0, 0, 0)):
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        self._chk(self.L.dspmap_stage_bin_points(self.h, pts.shape[0], 3, _ptr(pts), *[float(q) for q in quat]))

    def set_current_position(self, x, y, z):
        self._chk(self.L.dspmap_set_current_position(self.h, x, y, z))

    def predict(self, dx, dy, dz, dt):
        self._chk(self.L.dspmap_stage_predict(self.h, dx, dy, dz, dt))

    def map_update(self):
        self._chk(self.L.dspmap_stage_update(self.h))

    def add_newborn(self):
        self._chk(self.L.dspmap_stage_birth(self.h))

    def occupancy_resample(self):
        self._chk(self.L.dspmap_stage_resample(self.h))

    def pyramid_counts(self):
        out = np.zeros(self.NP, np.int32)
        self._chk(self.L.dspmap_get_pyramid_counts(self.h, _ptr(out)))
        return out

    def pyramid_candidates(self):
        """particles the last prediction tried to register per pyramid, before the cut (not clamped to the capacity)"""
        out = np.zeros(self.NP, np.int32)
        self._chk(self.L.dspmap_get_pyramid_candidates(self.h, _ptr(out)))
        return out

    def observations(self):
        obs = np.zeros((self.NP, 100, 5), np.float32)
        cnt = np.zeros(self.NP, np.int32)
        ml = np.zeros(self.NP, np.float32)
        e = C.c_float()
        self._chk(self.L.dspmap_get_observations(self.h, _ptr(obs), _ptr(cnt), _ptr(ml), C.byref(e)))
        return obs, cnt, ml, e.value
