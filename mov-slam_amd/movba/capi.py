"""ctypes binding of libmovba.so (include/movba.h) — the Python-side stand-in for the
C++ adapter (mov-slam_amd/host/Optimizer.cc) used by tests/ and bench.py.

There is no CPU fallback: if the shared library is missing, or no HIP device is
visible, every entry point raises (MovbaError) instead of computing anything here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MOVBA_LIB selects another build of the same library (diagnostic builds, e.g. -DMOVBA_CLOCK_STAMP)
LIB_PATH = os.environ.get("MOVBA_LIB") or os.path.join(os.path.dirname(_HERE), "libmovba.so")
# the TEST build of the same sources (-DMOVBA_TEST_HOOKS: per-handle switches through movba_test_hook; tests only)
HOOKS_LIB_PATH = os.path.join(os.path.dirname(_HERE), "libmovba_hooks.so")

MAX_TRACE = 128
NKERNELS = 6
OK, STOPPED, NO_FIXED, EMPTY, ERR_ARG, ERR_HIP, ERR_STATE, ERR_DEVICE_WAIT, ERR_TOO_LARGE = 0, 1, 2, 3, -1, -2, -3, -4, -5
SINGULAR = 4
FLAG_STALE_ERROR_QUIRK = 1

_d = C.POINTER(C.c_double)
_i = C.POINTER(C.c_int32)
_u = C.POINTER(C.c_uint8)
_q = C.POINTER(C.c_uint64)
_f = C.POINTER(C.c_float)
_h = C.POINTER(C.c_int16)


class MovbaError(RuntimeError):
    pass


class LbaDesc(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("poses", _d), ("pose_fixed", _u), ("points", _d), ("edge_pose", _i), ("edge_point", _i),
                ("obs", _d), ("inv_sigma2", _d),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("huber_delta", C.c_double), ("chi2_gate", C.c_double),
                ("max_iters", C.c_int32), ("max_trials", C.c_int32), ("flags", C.c_uint32), ("stop", _u),
                ("obs_right", _d), ("bf", C.c_double), ("cam_kf", _d), ("bf_kf", _d)]


class LbaResult(C.Structure):
    _fields_ = [("poses", _d), ("points", _d), ("chi2", _d), ("outlier", _u),
                ("status", C.c_int32), ("iters_done", C.c_int32), ("n_solves", C.c_int32),
                ("n_outliers", C.c_int32), ("pcg_iters", C.c_int32), ("last_rejected", C.c_int32),
                ("lambda_", C.c_double), ("cost0", C.c_double), ("cost", C.c_double),
                ("n_trace", C.c_int32),
                ("tr_lambda", C.c_double * MAX_TRACE), ("tr_f0", C.c_double * MAX_TRACE),
                ("tr_f1", C.c_double * MAX_TRACE), ("tr_rho", C.c_double * MAX_TRACE),
                ("tr_accept", C.c_int32 * MAX_TRACE), ("tr_pcg_iters", C.c_int32 * MAX_TRACE),
                ("n_direct", C.c_int32), ("direct_from", C.c_int32), ("n_chol_fail", C.c_int32), ("n_pcg_giveups", C.c_int32),
                ("n_sync_timeouts", C.c_int32), ("n_band", C.c_int32)]


class Options(C.Structure):
    _fields_ = [("pcg_rel_tol", C.c_double), ("pcg_max_iters", C.c_int32), ("run_ahead", C.c_int32),
                ("profile", C.c_int32), ("pcg_coarse", C.c_int32), ("host_wait", C.c_int32), ("pcg_spill", C.c_int32), ("solver", C.c_int32), ("reorder", C.c_int32), ("pad_o", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("name", C.c_char_p * NKERNELS), ("ms", C.c_double * NKERNELS), ("launches", C.c_int64 * NKERNELS),
                ("upload_ms", C.c_double), ("structure_ms", C.c_double), ("download_ms", C.c_double)]


class StructureInfo(C.Structure):
    _fields_ = [("n_free", C.c_int32), ("n_pairs", C.c_int32), ("n_entries", C.c_int64), ("n_items", C.c_int32),
                ("max_degree", C.c_int32), ("already_grouped", C.c_int32), ("pcg_on_chip", C.c_int32),
                ("pcg_overflow", C.c_int32), ("pcg_max_wave_entries", C.c_int32), ("n_row_entries", C.c_int32),
                ("n_sched_slots", C.c_int32), ("sched_items", C.c_int32), ("sched_max_permille", C.c_int32), ("slots_ok", C.c_int32),
                ("reordered", C.c_int32), ("pad_s", C.c_int32)]


class PoseDesc(C.Structure):
    _fields_ = [("n", C.c_int32), ("Xw", _d), ("obs", _d), ("inv_sigma2", _d),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("pose0", C.c_double * 7), ("huber_delta", C.c_double), ("chi2_gate", C.c_double),
                ("rounds", C.c_int32), ("its_per_round", C.c_int32), ("ransac_iters", C.c_int32), ("ransac_seed", C.c_uint32),
                ("confidence", C.c_double), ("lo_iters", C.c_int32), ("pad_p", C.c_int32)]


class PoseResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("outlier", _u), ("chi2", _d), ("n_inliers", C.c_int32), ("status", C.c_int32),
                ("ransac_inliers", C.c_int32), ("lm_iters", C.c_int32), ("ransac_pose", C.c_double * 7),
                ("ransac_samples_used", C.c_int32), ("lo_accepted", C.c_int32), ("lo_inliers", C.c_int32), ("pad_q", C.c_int32)]


class TriDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_pairs", C.c_int32), ("poses", _d), ("cam", _d), ("bf", _d), ("b", _d),
                ("pair_view", _i), ("pair_ptr", _i), ("obs1", _d), ("obs2", _d), ("ur1", _d), ("ur2", _d),
                ("depth1", _d), ("depth2", _d), ("reproj_gate", C.c_double), ("far_threshold", C.c_double)]


class TriResult(C.Structure):
    _fields_ = [("points", _d), ("code", _u), ("n_accepted", C.c_int32), ("status", C.c_int32)]


class TwoViewDesc(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("ransac_iters", C.c_int32), ("obs1", _d), ("obs2", _d),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("threshold", C.c_double), ("confidence", C.c_double), ("sigma", C.c_double), ("min_parallax_deg", C.c_double),
                ("max_depth", C.c_double), ("min_triangulated", C.c_int32), ("ransac_seed", C.c_uint32)]


class TwoViewResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("E", C.c_double * 9), ("parallax_deg", C.c_double),
                ("outcome", C.c_int32), ("status", C.c_int32), ("n_inliers", C.c_int32), ("n_pass", C.c_int32),
                ("n_good", C.c_int32), ("samples_used", C.c_int32),
                ("inlier", _u), ("points", _d), ("good", _u), ("code", _u),
                ("hyp_nsol", _i), ("hyp_E", _d), ("hyp_loss", _d)]


class TwoViewLoInfo(C.Structure):
    _fields_ = [("loss0", C.c_double), ("loss", C.c_double), ("E0", C.c_double * 9), ("kept", C.c_int32), ("steps", C.c_int32),
                ("n_inliers0", C.c_int32), ("pad", C.c_int32)]


class InitMapDesc(C.Structure):
    _fields_ = [("n_matches", C.c_int32), ("max_iters", C.c_int32), ("max_trials", C.c_int32), ("min_tracked", C.c_int32),
                ("obs1", _d), ("obs2", _d), ("points", _d), ("use", _u), ("inv_sigma2_1", _d), ("inv_sigma2_2", _d),
                ("pose2", C.c_double * 7), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("huber_delta", C.c_double)]


class InitMapResult(C.Structure):
    _fields_ = [("pose", C.c_double * 7), ("points", _d), ("chi2", _d), ("median_depth", C.c_double), ("lambda_", C.c_double),
                ("cost0", C.c_double), ("cost", C.c_double), ("outcome", C.c_int32), ("status", C.c_int32), ("n_used", C.c_int32),
                ("iters_done", C.c_int32), ("n_solves", C.c_int32), ("last_rejected", C.c_int32), ("n_chol_fail", C.c_int32),
                ("pad", C.c_int32)]


class InitMapTrace(C.Structure):
    _fields_ = [("n_trace", C.c_int32), ("pad", C.c_int32),
                ("tr_lambda", C.c_double * MAX_TRACE), ("tr_f0", C.c_double * MAX_TRACE), ("tr_f1", C.c_double * MAX_TRACE),
                ("tr_rho", C.c_double * MAX_TRACE), ("tr_accept", C.c_int32 * MAX_TRACE)]


class ViewDesc(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_views", C.c_int32), ("points", _d), ("normals", _d), ("max_distance", _d),
                ("min_distance", _d), ("mode", _i), ("poses", _d), ("cam", _d), ("bf", _d), ("bounds", _d),
                ("log_scale_factor", _d), ("n_levels", _i), ("cos_limit", _d), ("q", _i), ("view_ptr", _i), ("item_point", _i)]


class ViewResult(C.Structure):
    _fields_ = [("code", _u), ("z", _d), ("uv", _d), ("dist", _d), ("view_cos", _d), ("level", _i), ("ur", _d),
                ("track_depth", _d), ("n_accepted", _i), ("median_depth", _d), ("status", C.c_int32), ("pad", C.c_int32)]


class NormalsDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_points", C.c_int32), ("n_levels", C.c_int32), ("pad", C.c_int32), ("poses", _d),
                ("points", _d), ("obs_ptr", _i), ("obs_view", _i), ("ref_view", _i), ("ref_level", _i), ("scale_factors", _d)]


class NormalsResult(C.Structure):
    _fields_ = [("normals", _d), ("max_distance", _d), ("min_distance", _d), ("status", C.c_int32), ("pad", C.c_int32)]


class CovisDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_points", C.c_int32), ("n_queries", C.c_int32), ("min_weight", C.c_int32),
                ("max_out", C.c_int32), ("pad", C.c_int32), ("obs_ptr", _i), ("obs_view", _i), ("eligible", _u),
                ("query_ptr", _i), ("query_point", _i), ("query_self", _i)]


class CovisResult(C.Structure):
    _fields_ = [("n_counted", _i), ("n_connected", _i), ("best_view", _i), ("best_weight", _i), ("out_view", _i),
                ("out_weight", _i), ("status", C.c_int32), ("pad", C.c_int32)]


class TrackDesc(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("n_queries", C.c_int32), ("view_ptr", _i), ("slot_track", _i), ("slot_taken", _u),
                ("slot_obs", _d), ("slot_ur", _d), ("slot_depth", _d), ("query_mode", _i), ("query_view", _i), ("query_ptr", _i),
                ("item_track", _i)]


class TrackResult(C.Structure):
    _fields_ = [("pair_ptr", _i), ("match_slot1", _i), ("match_slot2", _i), ("obs1", _d), ("obs2", _d), ("ur1", _d), ("ur2", _d),
                ("depth1", _d), ("depth2", _d), ("item_slot", _i), ("n_found", _i), ("n_matches", C.c_int32), ("status", C.c_int32)]


class ExpressDesc(C.Structure):
    _fields_ = [("n_images", C.c_int32), ("pad", C.c_int32), ("image", C.POINTER(C.c_void_p)), ("rows", _i), ("cols", _i),
                ("stride", _i), ("threshold", _i), ("item_ptr", _i), ("item_rect", _i), ("item_mode", _i), ("item_ref", _q)]


class ExpressResult(C.Structure):
    _fields_ = [("code", _u), ("desc", _q), ("count", _i), ("distance", _i), ("n_features", _i), ("status", C.c_int32),
                ("pad", C.c_int32)]


class AdvanceDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("pad", C.c_int32), ("image", C.POINTER(C.c_void_p)), ("rows", _i), ("cols", _i),
                ("stride", _i), ("threshold", _i), ("force_grid", _u), ("first_id", _i), ("prev_ptr", _i), ("prev_pt", _f),
                ("prev_mb", _i), ("prev_age", _i), ("prev_track", _i), ("prev_desc", _q), ("prev_coverage", _u), ("prev_cand", _i),
                ("mv_ptr", _i), ("mv_pt", _f), ("mv_dindx", _i), ("kp_ptr", _i), ("kp_rect", _i), ("grid_ptr", _i),
                ("grid_covered", _u)]


class AdvanceResult(C.Structure):
    _fields_ = [("order", _i), ("fate", _u), ("chosen_mv", _i), ("distance", _i), ("kp_found", _u), ("kp_code", _u),
                ("mov_cnt", _i), ("grid_ran", _u), ("next_id", _i), ("seg_ptr", _i), ("feat_src", _i), ("feat_track", _i),
                ("feat_pt", _f), ("feat_rect", _i), ("feat_age", _i), ("feat_desc", _q), ("status", C.c_int32), ("pad", C.c_int32)]


class MvRasterDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("pad", C.c_int32), ("rows", _i), ("cols", _i), ("coverage_threshold", _d), ("want_grid", _u),
                ("rec_ptr", _i), ("src_x", _h), ("src_y", _h), ("dst_x", _h), ("dst_y", _h), ("w", _u), ("h", _u), ("source", _i),
                ("ref", _i), ("q_ptr", _i), ("q_pt", _f)]


class MvRasterResult(C.Structure):
    _fields_ = [("kept_ptr", _i), ("kp_rect", _i), ("mv_pt", _f), ("mv_dindx", _i), ("rec_kept", _i), ("cand", _i), ("grid_ptr", _i),
                ("grid_covered", _u), ("cover_px", _i), ("coverage_area", _d), ("force_grid", _u), ("status", C.c_int32),
                ("pad", C.c_int32)]


class LkDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("pad", C.c_int32), ("prev_image", C.POINTER(C.c_void_p)), ("next_image", C.POINTER(C.c_void_p)),
                ("rows", _i), ("cols", _i), ("stride", _i), ("win", _i), ("pt_ptr", _i), ("pt", _f), ("max_level", C.c_int32),
                ("max_iter", C.c_int32), ("eps", C.c_double), ("min_eig_threshold", C.c_double)]


class LkResult(C.Structure):
    _fields_ = [("next_pt", _f), ("pt_status", _u), ("err", _f), ("exit_code", _u), ("keep", _u), ("kept_ptr", _i), ("kept_src", _i),
                ("status", C.c_int32), ("pad", C.c_int32)]


class StereoDesc(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("pad", C.c_int32), ("pt_ptr", _i), ("pt", _f), ("next_pt", _f), ("pt_status", _u), ("pt_un", _f),
                ("rows", _i), ("cols", _i), ("bf", _f), ("max_disparity", _f), ("th_depth", _f), ("cam", _f), ("select", _i), ("poses", _d),
                ("has_point", _u), ("max_row_diff", C.c_float), ("min_disparity", C.c_float), ("max_point", C.c_int32), ("pad2", C.c_int32)]


class StereoResult(C.Structure):
    _fields_ = [("u_right", _f), ("depth", _f), ("code", _u), ("n_stereo", _i), ("median_dist", _i), ("th_dist", _f), ("sel_ptr", _i),
                ("sel_src", _i), ("sel_new", _u), ("sel_cam", _f), ("sel_point", _d), ("status", C.c_int32), ("pad", C.c_int32)]


# (key, dtype, width, which count it is sized by) of movba_stereo_result
STEREO_ARRAYS = (("u_right", np.float32, 1, "pt"), ("depth", np.float32, 1, "pt"), ("code", np.uint8, 1, "pt"),
                 ("n_stereo", np.int32, 1, "frames"), ("median_dist", np.int32, 1, "frames"), ("th_dist", np.float32, 1, "frames"),
                 ("sel_ptr", np.int32, 1, "ptr"), ("sel_src", np.int32, 1, "pt"), ("sel_new", np.uint8, 1, "pt"),
                 ("sel_cam", np.float32, 3, "pt"), ("sel_point", np.float64, 3, "pt"))
# movba_stereo_desc::select, movba_stereo_result::code (MOVBA_STEREO_*) and the bound of a frame
STEREO_SELECT_NONE, STEREO_SELECT_ALL, STEREO_SELECT_CLOSE = 0, 1, 2
STEREO_OK = 1
STEREO_REJ_STATUS, STEREO_REJ_ROW, STEREO_REJ_DISPARITY, STEREO_REJ_FAR = range(16, 20)
MAX_STEREO_POINTS = 16384
# (key, dtype, width, which count it is sized by) of movba_lk_result
LK_ARRAYS = (("next_pt", np.float32, 2, "pt"), ("pt_status", np.uint8, 1, "pt"), ("err", np.float32, 1, "pt"),
             ("exit_code", np.uint8, 1, "pt"), ("keep", np.uint8, 1, "pt"), ("kept_ptr", np.int32, 1, "ptr"), ("kept_src", np.int32, 1, "pt"))
# movba_lk_result::exit_code (MOVBA_LK_*) and the bounds of movba_lk_desc
LK_EPS, LK_OSCILLATION, LK_MAX_ITER_RAN = 1, 2, 3
LK_REJ_START, LK_REJ_MIN_EIG, LK_REJ_LOOP = 16, 17, 18
LK_MAX_WIN, LK_MAX_LEVEL, LK_MAX_ITER, LK_MAX_PIXELS = 31, 3, 30, 1 << 26
# (key, dtype, width, which count it is sized by) of movba_mv_raster_result
MV_RASTER_ARRAYS = (("kept_ptr", np.int32, 1, "ptr"), ("kp_rect", np.int32, 4, "rec"), ("mv_pt", np.float32, 2, "rec"),
                    ("mv_dindx", np.int32, 1, "rec"), ("rec_kept", np.int32, 1, "rec"), ("cand", np.int32, 4, "q"),
                    ("grid_ptr", np.int32, 1, "ptr"), ("grid_covered", np.uint8, 1, "grid"), ("cover_px", np.int32, 1, "frames"),
                    ("coverage_area", np.float64, 1, "frames"), ("force_grid", np.uint8, 1, "frames"))
# the per-record fields of movba_mv_raster_desc
MV_RASTER_RECORD = (("src_x", np.int16), ("src_y", np.int16), ("dst_x", np.int16), ("dst_y", np.int16), ("w", np.uint8), ("h", np.uint8),
                    ("source", np.int32), ("ref", np.int32))
MAX_MV_RASTER_RECORDS = 1 << 20
# movba_advance_result::fate (MOVBA_ADV_*)
ADV_KEPT, ADV_COVERAGE = 1, 2
ADV_NO_MV, ADV_REJ_BOUNDS, ADV_LOST_CLAIM, ADV_FAR = range(16, 20)
MAX_ADVANCE_PREV = 16384
# (key, dtype, width, which count it is sized by) of movba_advance_result
ADVANCE_ARRAYS = (("order", np.int32, 1, "prev"), ("fate", np.uint8, 1, "prev"), ("chosen_mv", np.int32, 1, "prev"),
                  ("distance", np.int32, 1, "prev"), ("kp_found", np.uint8, 1, "kps"), ("kp_code", np.uint8, 1, "kps"),
                  ("mov_cnt", np.int32, 1, "frames"), ("grid_ran", np.uint8, 1, "frames"), ("next_id", np.int32, 1, "frames"),
                  ("seg_ptr", np.int32, 1, "seg"), ("feat_src", np.int32, 1, "cap"), ("feat_track", np.int32, 1, "cap"),
                  ("feat_pt", np.float32, 2, "cap"), ("feat_rect", np.int32, 4, "cap"), ("feat_age", np.int32, 1, "cap"),
                  ("feat_desc", np.uint64, 4, "cap"))
ADVANCE_PREV = (("prev_pt", np.float32, 2), ("prev_mb", np.int32, 2), ("prev_age", np.int32, 1), ("prev_track", np.int32, 1),
                ("prev_desc", np.uint64, 4), ("prev_coverage", np.uint8, 1), ("prev_cand", np.int32, 4))
# movba_express_desc::item_mode and movba_express_result::code (MOVBA_EX_*)
EX_DETECT, EX_DESCRIBE = 0, 1
EX_FEATURE, EX_DESCRIBED = 1, 2
EX_REJ_BOUNDS, EX_REJ_SHAPE, EX_REJ_FLAT, EX_REJ_NO_EDGE = range(16, 20)
MAX_EXPRESS_IMAGES = 1024
MAX_EXPRESS_ITEMS = 1 << 22
EXPRESS_ARRAYS = (("code", np.uint8, 1), ("desc", np.uint64, 4), ("count", np.int32, 1), ("distance", np.int32, 1))
# movba_track_desc::query_mode (MOVBA_TM_*)
TM_TRIANGULATION, TM_LOOKUP = 0, 1
MAX_TRACK_SLOTS = 16384
MAX_TRACK_QUERIES = 4096
TRACK_INT_ARRAYS = ("pair_ptr", "match_slot1", "match_slot2", "item_slot", "n_found")
TRACK_PAYLOAD = (("obs1", "obs"), ("obs2", "obs"), ("ur1", "ur"), ("ur2", "ur"), ("depth1", "depth"), ("depth2", "depth"))
MAX_COVIS_VIEWS = 8192
MAX_COVIS_QUERIES = 4096
COVIS_ARRAYS = ("n_counted", "n_connected", "best_view", "best_weight", "out_view", "out_weight")
MAX_INIT_MAP_ITERS = 100
# movba_init_map_result::outcome (MOVBA_IM_*)
IM_OK, IM_NEG_DEPTH, IM_FEW_TRACKED = 0, 1, 2
MAX_TWO_VIEW_ITERS = 1024
MAX_TWO_VIEW_LO_ITERS = 32
MAX_TWO_VIEW_BATCH = 1024
MAX_TWO_VIEW_MATCHES = 32768
# movba_two_view_result::outcome (MOVBA_TV_*) and ::code (MOVBA_TV_CHK_*)
TV_OK, TV_NO_MODEL, TV_FEW_GOOD, TV_LOW_PARALLAX = 0, 1, 2, 3
TV_CHK_NONE, TV_CHK_GOOD, TV_CHK_LOW_PARALLAX = 0, 1, 2
(TV_CHK_REJ_NOT_INLIER, TV_CHK_REJ_W0, TV_CHK_REJ_BEHIND1, TV_CHK_REJ_BEHIND2, TV_CHK_REJ_REPROJ1,
 TV_CHK_REJ_REPROJ2) = range(16, 22)

# movba_tri_result::code (MOVBA_TRI_*): accepted ...
TRI_DLT, TRI_STEREO1, TRI_STEREO2 = 1, 2, 3
# ... and rejected, in the order the reference tests
(TRI_REJ_W0, TRI_REJ_PARALLAX, TRI_REJ_DEPTH, TRI_REJ_BEHIND1, TRI_REJ_BEHIND2, TRI_REJ_REPROJ1, TRI_REJ_REPROJ2,
 TRI_REJ_ZERO_DIST, TRI_REJ_FAR) = range(16, 25)
TRI_ACCEPTED = (TRI_DLT, TRI_STEREO1, TRI_STEREO2)

# movba_view_desc::mode (MOVBA_VIEW_*)
VIEW_FRUSTUM, VIEW_FUSE, VIEW_DEPTH = 0, 1, 2
MAX_VIEW_BATCH = 4096
# movba_view_result::code (MOVBA_VP_*): accepted ...
VP_VISIBLE, VP_FUSE_CANDIDATE, VP_DEPTH_ITEM = 1, 2, 3
# ... and rejected, in the order the reference tests
VP_REJ_BEHIND, VP_REJ_U, VP_REJ_V, VP_REJ_IMAGE, VP_REJ_DIST, VP_REJ_ANGLE = range(16, 22)
VP_ACCEPTED = (VP_VISIBLE, VP_FUSE_CANDIDATE, VP_DEPTH_ITEM)

EXPORTS = ["movba_version", "movba_status_string", "movba_create", "movba_destroy", "movba_lba_solve",
           "movba_lba_upload", "movba_lba_reset", "movba_lba_run", "movba_lba_download",
           "movba_lba_export_poses_device", "movba_lba_set_pose_export", "movba_get_profile", "movba_reset_profile",
           "movba_structure_probe", "movba_pose_opt", "movba_set_profile_mask", "movba_lba_run_batch", "movba_pose_ransac_samples",
           "movba_host_alloc", "movba_host_free", "movba_dense_plan_probe", "movba_pose_opt_batch", "movba_lba_marginals", "movba_triangulate",
           "movba_two_view", "movba_two_view_samples", "movba_two_view_lo", "movba_init_map", "movba_view_points",
           "movba_point_normals", "movba_lba_point_normals", "movba_covisibility", "movba_track_match", "movba_express",
           "movba_express_grid", "movba_advance", "movba_mv_raster", "movba_lk_track", "movba_stereo_points"]

_libs = {False: None, True: None}


def _one_hip_runtime():
    """A process must hold ONE copy of the HIP runtime.  libmovba.so needs `libamdhip64.so.7` (found in /opt/rocm); torch's
    libtorch_hip.so needs `libamdhip64.so` (found in torch/lib by its rpath: another FILE with the same soname, 7).  Loaded
    first, torch's copy satisfies libmovba's soname; loaded second, it is mapped beside ROCm's copy, and the second runtime
    finds no device ("no ROCm-capable device is detected": profiles/r03p_hip_runtime_copies.log).  So when torch is installed
    its copy is mapped (RTLD_GLOBAL) before libmovba.so — without importing torch — and both bind to that one whichever is
    imported first; without torch (the C++ adapter inside MoV-SLAM) ROCm's own copy is the only one there is."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib(hooks: bool = False):
    """Load libmovba.so (hooks: the test build, libmovba_hooks.so); raise loudly when the HIP extension has not been built."""
    if _libs[hooks] is None:
        path = HOOKS_LIB_PATH if hooks else LIB_PATH
        if not os.path.exists(path):
            raise MovbaError(f"{path} not found: build it with `make -C mov-slam_amd/csrc` "
                             "(or __graft_entry__.build()); there is no CPU fallback")
        _one_hip_runtime()
        L = C.CDLL(path)
        if hooks:
            L.movba_test_hook.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]
        L.movba_status_string.restype = C.c_char_p
        L.movba_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(Options)]
        L.movba_destroy.argtypes = [C.c_void_p]
        L.movba_destroy.restype = None
        for fn in ("movba_lba_upload",):
            getattr(L, fn).argtypes = [C.c_void_p, C.POINTER(LbaDesc)]
        L.movba_lba_solve.argtypes = [C.c_void_p, C.POINTER(LbaDesc), C.POINTER(LbaResult)]
        L.movba_lba_run.argtypes = [C.c_void_p]
        L.movba_lba_reset.argtypes = [C.c_void_p]
        L.movba_lba_download.argtypes = [C.c_void_p, C.POINTER(LbaResult)]
        L.movba_lba_export_poses_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.movba_lba_set_pose_export.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.movba_get_profile.argtypes = [C.c_void_p, C.POINTER(Profile)]
        L.movba_reset_profile.argtypes = [C.c_void_p]
        L.movba_set_profile_mask.argtypes = [C.c_void_p, C.c_int32]
        L.movba_structure_probe.argtypes = [C.POINTER(LbaDesc), C.POINTER(StructureInfo), _i, _i]
        L.movba_pose_opt.argtypes = [C.c_void_p, C.POINTER(PoseDesc), C.POINTER(PoseResult)]
        L.movba_pose_opt_batch.argtypes = [C.c_void_p, C.POINTER(PoseDesc), C.POINTER(PoseResult), C.c_int32]
        L.movba_lba_run_batch.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
        L.movba_lba_marginals.argtypes = [C.c_void_p, C.c_double, _d, _d]
        L.movba_triangulate.argtypes = [C.c_void_p, C.POINTER(TriDesc), C.POINTER(TriResult)]
        L.movba_pose_ransac_samples.argtypes = [C.c_int32, C.c_int32, C.c_uint32, _i]
        L.movba_two_view.argtypes = [C.c_void_p, C.POINTER(TwoViewDesc), C.POINTER(TwoViewResult), C.c_int32]
        L.movba_two_view_samples.argtypes = [C.c_int32, C.c_int32, C.c_uint32, _i]
        L.movba_two_view_lo.argtypes = [C.c_void_p, C.POINTER(TwoViewDesc), C.POINTER(TwoViewResult), C.c_int32, C.c_int32,
                                        C.POINTER(TwoViewLoInfo)]
        L.movba_init_map.argtypes = [C.c_void_p, C.POINTER(InitMapDesc), C.POINTER(InitMapResult), C.c_int32, C.POINTER(InitMapTrace)]
        L.movba_view_points.argtypes = [C.c_void_p, C.POINTER(ViewDesc), C.POINTER(ViewResult)]
        L.movba_point_normals.argtypes = [C.c_void_p, C.POINTER(NormalsDesc), C.POINTER(NormalsResult)]
        L.movba_lba_point_normals.argtypes = [C.c_void_p, _i, _i, _d, C.c_int32, _u, _d, _d, _d]
        L.movba_covisibility.argtypes = [C.c_void_p, C.POINTER(CovisDesc), C.POINTER(CovisResult)]
        L.movba_track_match.argtypes = [C.c_void_p, C.POINTER(TrackDesc), C.POINTER(TrackResult)]
        L.movba_express.argtypes = [C.c_void_p, C.POINTER(ExpressDesc), C.POINTER(ExpressResult)]
        L.movba_express_grid.argtypes = [C.c_int32, C.c_int32, _i, C.c_int32]
        L.movba_advance.argtypes = [C.c_void_p, C.POINTER(AdvanceDesc), C.POINTER(AdvanceResult)]
        L.movba_mv_raster.argtypes = [C.c_void_p, C.POINTER(MvRasterDesc), C.POINTER(MvRasterResult)]
        L.movba_lk_track.argtypes = [C.c_void_p, C.POINTER(LkDesc), C.POINTER(LkResult)]
        L.movba_stereo_points.argtypes = [C.c_void_p, C.POINTER(StereoDesc), C.POINTER(StereoResult)]
        L.movba_host_alloc.argtypes = [C.c_size_t]
        L.movba_host_alloc.restype = C.c_void_p
        L.movba_dense_plan_probe.argtypes = [C.c_int32, C.c_int32, C.c_int32, _i, _i, C.c_int32, _i, C.c_int32]
        L.movba_host_free.argtypes = [C.c_void_p]
        L.movba_host_free.restype = None
        _libs[hooks] = L
    return _libs[hooks]


def status_string(s: int) -> str:
    return lib().movba_status_string(s).decode()


def _p(a, t):
    return a.ctypes.data_as(t)


def make_desc(w, flags=FLAG_STALE_ERROR_QUIRK, stop=None, max_iters=None, max_trials=0):
    """Flattened window (movba.synth.Window or anything with the same fields) -> movba_lba_desc."""
    keep = dict(
        poses=np.ascontiguousarray(w.poses, np.float64), fixed=np.ascontiguousarray(w.pose_fixed, np.uint8),
        points=np.ascontiguousarray(w.points, np.float64), ep=np.ascontiguousarray(w.edge_pose, np.int32),
        el=np.ascontiguousarray(w.edge_point, np.int32), obs=np.ascontiguousarray(w.obs, np.float64),
        isg=np.ascontiguousarray(w.inv_sigma2, np.float64))
    d = LbaDesc()
    d.n_poses, d.n_points, d.n_edges = len(keep["poses"]), len(keep["points"]), len(keep["ep"])
    d.poses = _p(keep["poses"], _d); d.pose_fixed = _p(keep["fixed"], _u); d.points = _p(keep["points"], _d)
    d.edge_pose = _p(keep["ep"], _i); d.edge_point = _p(keep["el"], _i)
    d.obs = _p(keep["obs"], _d); d.inv_sigma2 = _p(keep["isg"], _d)
    d.fx, d.fy, d.cx, d.cy = w.cam
    d.huber_delta, d.chi2_gate = w.huber_delta, w.chi2_gate
    d.max_iters = w.max_iters if max_iters is None else max_iters
    d.flags = flags
    d.max_trials = max_trials
    if stop is not None:
        keep["stop"] = stop
        d.stop = _p(stop, _u)
    if getattr(w, "obs_right", None) is not None:
        keep["obs_right"] = np.ascontiguousarray(w.obs_right, np.float64)
        d.obs_right = _p(keep["obs_right"], _d)
        d.bf = float(w.bf)
    if getattr(w, "cam_kf", None) is not None:           # intrinsics by keyframe (n_poses x 4)
        keep["cam_kf"] = np.ascontiguousarray(w.cam_kf, np.float64)
        assert keep["cam_kf"].shape == (d.n_poses, 4)
        d.cam_kf = _p(keep["cam_kf"], _d)
    if getattr(w, "bf_kf", None) is not None:
        keep["bf_kf"] = np.ascontiguousarray(w.bf_kf, np.float64)
        assert keep["bf_kf"].shape == (d.n_poses,)
        d.bf_kf = _p(keep["bf_kf"], _d)
    return d, keep


def _pose_desc(Xw, obs, pose0, cam, huber_delta, chi2_gate, rounds=4, its=10, inv_sigma2=None, ransac_iters=0, ransac_seed=1,
               confidence=0.0, lo_iters=0):
    """One frame -> (movba_pose_desc, movba_pose_result with its output arrays, the arrays both point into)."""
    keep = dict(Xw=np.ascontiguousarray(Xw, np.float64), obs=np.ascontiguousarray(obs, np.float64))
    n = len(keep["Xw"])
    d = PoseDesc()
    d.n = n; d.Xw = _p(keep["Xw"], _d); d.obs = _p(keep["obs"], _d)
    if inv_sigma2 is not None:
        keep["isg"] = np.ascontiguousarray(inv_sigma2, np.float64); d.inv_sigma2 = _p(keep["isg"], _d)
    d.fx, d.fy, d.cx, d.cy = cam
    d.pose0 = (C.c_double * 7)(*pose0)
    d.huber_delta, d.chi2_gate, d.rounds, d.its_per_round = huber_delta, chi2_gate, rounds, its
    d.ransac_iters, d.ransac_seed = ransac_iters, ransac_seed
    d.confidence, d.lo_iters = confidence, lo_iters
    keep["outlier"] = np.zeros(n, np.uint8); keep["chi2"] = np.zeros(n)
    r = PoseResult(); r.outlier = _p(keep["outlier"], _u); r.chi2 = _p(keep["chi2"], _d)
    return d, r, keep


def _pose_dict(r, keep, status):
    return dict(status=status, n_inliers=r.n_inliers, pose=np.array(r.pose[:]), outlier=keep["outlier"], chi2=keep["chi2"],
                ransac_inliers=r.ransac_inliers, ransac_pose=np.array(r.ransac_pose[:]), lm_iters=r.lm_iters,
                ransac_samples_used=r.ransac_samples_used, lo_accepted=r.lo_accepted, lo_inliers=r.lo_inliers)


def tri_desc(views, pairs, matches, reproj_gate=5.0, far_threshold=0.0):
    """views dict(poses (V, 7), cam (V, 4), optional bf, b (V,)), pairs dict(pair_view (P, 2), pair_ptr (P + 1,)), matches
    dict(obs1, obs2 (M, 2), optional ur1, ur2, depth1, depth2 (M,)) -> (movba_tri_desc, the arrays it points into)."""
    keep = {}
    d = TriDesc()

    def arr(src, key, dtype, ptr):
        a = src.get(key)
        if a is None:
            return
        keep[key] = np.ascontiguousarray(a, dtype)
        setattr(d, key, _p(keep[key], ptr))

    for key in ("poses", "cam", "bf", "b"):
        arr(views, key, np.float64, _d)
    for key in ("pair_view", "pair_ptr"):
        arr(pairs, key, np.int32, _i)
    for key in ("obs1", "obs2", "ur1", "ur2", "depth1", "depth2"):
        arr(matches, key, np.float64, _d)
    d.n_views = len(keep["poses"]) if "poses" in keep else 0
    d.n_pairs = len(keep["pair_view"]) if "pair_view" in keep else 0
    d.reproj_gate, d.far_threshold = reproj_gate, far_threshold
    return d, keep


def structure_probe(w):
    d, keep = make_desc(w)
    info = StructureInfo()
    perm = np.zeros(d.n_edges, np.int32); fidx = np.zeros(d.n_poses, np.int32)
    rc = lib().movba_structure_probe(C.byref(d), C.byref(info), _p(perm, _i), _p(fidx, _i))
    if rc < 0:
        raise MovbaError(f"movba_structure_probe: {status_string(rc)}")
    return dict(status=rc, n_free=info.n_free, n_pairs=info.n_pairs, n_entries=info.n_entries, n_items=info.n_items,
                max_degree=info.max_degree, already_grouped=bool(info.already_grouped), pcg_on_chip=bool(info.pcg_on_chip),
                pcg_overflow=bool(info.pcg_overflow), pcg_max_wave_entries=info.pcg_max_wave_entries,
                n_row_entries=info.n_row_entries, n_sched_slots=info.n_sched_slots, sched_items=info.sched_items,
                sched_max_permille=info.sched_max_permille, slots_ok=bool(info.slots_ok), reordered=bool(info.reordered), perm=perm, free_index=fidx)


def dense_plan(nt: int, max_groups: int = 0, max_slots: int = 0):
    """Static schedule of the one-launch direct solver for nt block columns (host only): dict(ok, G, slots, task_ptr, tasks)
    with tasks as rows (op, slot, I, K, k, pad0, pad1)."""
    info = np.zeros(4, np.int32)
    lib().movba_dense_plan_probe(nt, max_groups, max_slots, _p(info, _i), None, 0, None, 0)
    if not info[0]:
        return dict(ok=False, G=0, slots=0, task_ptr=np.zeros(1, np.int32), tasks=np.zeros((0, 7), np.int32), tasks8=np.zeros((0, 8), np.int32))
    tp = np.zeros(info[1] + 1, np.int32); tk = np.zeros((info[3], 8), np.int32)
    lib().movba_dense_plan_probe(nt, max_groups, max_slots, _p(info, _i), _p(tp, _i), len(tp), _p(tk, _i), info[3])
    return dict(ok=True, G=int(info[1]), slots=int(info[2]), task_ptr=tp, tasks=tk[:, :7], tasks8=tk)


def ransac_samples(n: int, n_hyp: int, seed: int) -> np.ndarray:
    """The minimal samples movba_pose_opt draws (host only): (n_hyp, 3) match indices."""
    out = np.zeros((n_hyp, 3), np.int32)
    rc = lib().movba_pose_ransac_samples(n, n_hyp, seed, _p(out, _i))
    if rc != OK:
        raise MovbaError(f"movba_pose_ransac_samples: {status_string(rc)}")
    return out


def two_view_samples(n_matches: int, n_hyp: int, seed: int) -> np.ndarray:
    """The minimal samples movba_two_view draws (host only): (n_hyp, 5) match indices."""
    out = np.zeros((n_hyp, 5), np.int32)
    rc = lib().movba_two_view_samples(n_matches, n_hyp, seed, _p(out, _i))
    if rc != OK:
        raise MovbaError(f"movba_two_view_samples: {status_string(rc)}")
    return out


TWO_VIEW_DEFAULTS = dict(threshold=1.0, confidence=0.999, sigma=1.0, min_parallax_deg=1.0, max_depth=50.0, min_triangulated=50,
                         ransac_iters=256, ransac_seed=1)


def two_view_desc(pair, alloc=np.zeros, diagnostics=False, alloc_by=None):
    """One frame pair - dict(obs1, obs2 (M, 2), cam (fx, fy, cx, cy), optional TWO_VIEW_DEFAULTS keys) ->
    (movba_two_view_desc, movba_two_view_result with its output arrays, the arrays both point into).  alloc_by: allocators of
    single result arrays by name, where they differ from alloc."""
    mk = lambda key, shape, dtype: (alloc_by or {}).get(key, alloc)(shape, dtype)
    keep = dict(obs1=np.ascontiguousarray(pair["obs1"], np.float64).reshape(-1, 2),
                obs2=np.ascontiguousarray(pair["obs2"], np.float64).reshape(-1, 2))
    m = len(keep["obs1"])
    d = TwoViewDesc()
    d.n_matches = m; d.obs1 = _p(keep["obs1"], _d); d.obs2 = _p(keep["obs2"], _d)
    d.fx, d.fy, d.cx, d.cy = pair["cam"]
    for key, val in TWO_VIEW_DEFAULTS.items():
        setattr(d, key, pair.get(key, val))
    keep.update(inlier=mk("inlier", (m,), np.uint8), points=mk("points", (m, 3), np.float64), good=mk("good", (m,), np.uint8),
                code=mk("code", (m,), np.uint8))
    r = TwoViewResult()
    r.inlier = _p(keep["inlier"], _u); r.points = _p(keep["points"], _d); r.good = _p(keep["good"], _u); r.code = _p(keep["code"], _u)
    if diagnostics:
        nh = d.ransac_iters
        keep.update(hyp_nsol=np.zeros(nh, np.int32), hyp_E=np.zeros((nh, 10, 3, 3)), hyp_loss=np.zeros((nh, 10)))
        r.hyp_nsol = _p(keep["hyp_nsol"], _i); r.hyp_E = _p(keep["hyp_E"], _d); r.hyp_loss = _p(keep["hyp_loss"], _d)
    return d, r, keep


INIT_MAP_DEFAULTS = dict(max_iters=20, max_trials=0, min_tracked=50, huber_delta=float(np.sqrt(np.float32(5.0))))


def init_map_desc(pair, alloc=np.zeros, chi2=True, alloc_by=None):
    """One frame pair - dict(obs1, obs2 (M, 2), points (M, 3), pose2 (7,), cam (fx, fy, cx, cy), optional use (M,),
    inv_sigma2_1, inv_sigma2_2 (M,) and the keys of INIT_MAP_DEFAULTS) -> (movba_init_map_desc, movba_init_map_result with its
    output arrays, the arrays both point into).  alloc_by: as two_view_desc."""
    mk = lambda key, shape, dtype: (alloc_by or {}).get(key, alloc)(shape, dtype)
    keep = dict(obs1=np.ascontiguousarray(pair["obs1"], np.float64).reshape(-1, 2),
                obs2=np.ascontiguousarray(pair["obs2"], np.float64).reshape(-1, 2),
                points_in=np.ascontiguousarray(pair["points"], np.float64).reshape(-1, 3))
    m = len(keep["obs1"])
    d = InitMapDesc()
    d.n_matches = m; d.obs1 = _p(keep["obs1"], _d); d.obs2 = _p(keep["obs2"], _d); d.points = _p(keep["points_in"], _d)
    if pair.get("use") is not None:
        keep["use"] = np.ascontiguousarray(pair["use"], np.uint8)
        d.use = _p(keep["use"], _u)
    for key in ("inv_sigma2_1", "inv_sigma2_2"):
        if pair.get(key) is not None:
            keep[key] = np.ascontiguousarray(pair[key], np.float64)
            setattr(d, key, _p(keep[key], _d))
    d.pose2 = (C.c_double * 7)(*[float(v) for v in pair["pose2"]])
    d.fx, d.fy, d.cx, d.cy = pair["cam"]
    for key, val in INIT_MAP_DEFAULTS.items():
        setattr(d, key, pair.get(key, val))
    keep["points"] = mk("points", (m, 3), np.float64)
    r = InitMapResult()
    r.points = _p(keep["points"], _d)
    if chi2:
        keep["chi2"] = mk("chi2", (m, 2), np.float64)
        r.chi2 = _p(keep["chi2"], _d)
    return d, r, keep


VIEW_DEFAULTS = dict(bf=0.0, bounds=(0.0, 0.0, 0.0, 0.0), log_scale_factor=float(np.log(1.2)), n_levels=8, cos_limit=0.5, q=2)
# the optional per-item arrays of movba_view_result: name -> (entries per item, dtype)
VIEW_ITEM_ARRAYS = dict(z=(1, np.float64), uv=(2, np.float64), dist=(1, np.float64), view_cos=(1, np.float64), level=(1, np.int32),
                        ur=(1, np.float64), track_depth=(1, np.float64))


def view_desc(points, views):
    """points dict(points (N, 3), optional normals (N, 3), max_distance, min_distance (N,)), views: list of dicts with mode
    (VIEW_*), pose (7,), cam (4,), items (indices into the point table) and optionally the keys of VIEW_DEFAULTS ->
    (movba_view_desc, the arrays it points into).  The per-view arrays a mode does not read are still passed, with the
    defaults."""
    keep = dict(points=np.ascontiguousarray(points["points"], np.float64).reshape(-1, 3))
    d = ViewDesc()
    d.n_points = len(keep["points"]); d.points = _p(keep["points"], _d)
    for key in ("normals", "max_distance", "min_distance"):
        if points.get(key) is not None:
            keep[key] = np.ascontiguousarray(points[key], np.float64)
            setattr(d, key, _p(keep[key], _d))
    nv = len(views)
    d.n_views = nv
    get = lambda v, key: v.get(key, VIEW_DEFAULTS[key])
    keep["mode"] = np.array([v["mode"] for v in views], np.int32).reshape(nv)
    keep["poses"] = np.array([v["pose"] for v in views], np.float64).reshape(nv, 7)
    keep["cam"] = np.array([v["cam"] for v in views], np.float64).reshape(nv, 4)
    keep["bf"] = np.array([get(v, "bf") for v in views], np.float64).reshape(nv)
    keep["bounds"] = np.array([get(v, "bounds") for v in views], np.float64).reshape(nv, 4)
    keep["log_scale_factor"] = np.array([get(v, "log_scale_factor") for v in views], np.float64).reshape(nv)
    keep["n_levels"] = np.array([get(v, "n_levels") for v in views], np.int32).reshape(nv)
    keep["cos_limit"] = np.array([get(v, "cos_limit") for v in views], np.float64).reshape(nv)
    keep["q"] = np.array([get(v, "q") for v in views], np.int32).reshape(nv)
    items = [np.asarray(v["items"], np.int32).reshape(-1) for v in views]
    keep["view_ptr"] = np.concatenate([[0], np.cumsum([len(i) for i in items])]).astype(np.int32)
    keep["item_point"] = np.ascontiguousarray(np.concatenate(items) if items else np.zeros(0), np.int32)
    for key in ("poses", "cam", "bf", "bounds", "log_scale_factor", "cos_limit"):
        setattr(d, key, _p(keep[key], _d))
    for key in ("mode", "n_levels", "q", "view_ptr", "item_point"):
        setattr(d, key, _p(keep[key], _i))
    return d, keep


def view_result(n_items, n_views, alloc=np.zeros, arrays=tuple(VIEW_ITEM_ARRAYS)):
    """-> (movba_view_result with its output arrays, the arrays it points into); arrays: the optional per-item arrays asked
    for (the others stay NULL)."""
    keep = dict(code=alloc((n_items,), np.uint8), n_accepted=alloc((n_views,), np.int32), median_depth=alloc((n_views,), np.float64))
    r = ViewResult()
    r.code = _p(keep["code"], _u); r.n_accepted = _p(keep["n_accepted"], _i); r.median_depth = _p(keep["median_depth"], _d)
    for key in arrays:
        width, dtype = VIEW_ITEM_ARRAYS[key]
        keep[key] = alloc((n_items, width) if width > 1 else (n_items,), dtype)
        setattr(r, key, _p(keep[key], _i if dtype == np.int32 else _d))
    return r, keep


def normals_desc(points, views, lists, ref_view, ref_level, scale_factors):
    """points (N, 3), views (V, 7) poses Tcw, lists: one sequence of view indices per point (its observers, in the order they
    are summed), ref_view, ref_level (N,), scale_factors (L,) -> (movba_normals_desc, the arrays it points into)."""
    keep = dict(points=np.ascontiguousarray(points, np.float64).reshape(-1, 3), poses=np.ascontiguousarray(views, np.float64).reshape(-1, 7),
                ref_view=np.ascontiguousarray(ref_view, np.int32).reshape(-1), ref_level=np.ascontiguousarray(ref_level, np.int32).reshape(-1),
                scale_factors=np.ascontiguousarray(scale_factors, np.float64).reshape(-1))
    lists = [np.asarray(l, np.int32).reshape(-1) for l in lists]
    keep["obs_ptr"] = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    keep["obs_view"] = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32)
    d = NormalsDesc()
    d.n_views, d.n_points, d.n_levels = len(keep["poses"]), len(keep["points"]), len(keep["scale_factors"])
    for key in ("poses", "points", "scale_factors"):
        setattr(d, key, _p(keep[key], _d))
    for key in ("obs_ptr", "obs_view", "ref_view", "ref_level"):
        setattr(d, key, _p(keep[key], _i))
    return d, keep


def normals_result(n_points, alloc=np.zeros):
    """-> (movba_normals_result with its output arrays, the arrays it points into)"""
    keep = dict(normals=alloc((n_points, 3), np.float64), max_distance=alloc((n_points,), np.float64), min_distance=alloc((n_points,), np.float64))
    r = NormalsResult()
    r.normals = _p(keep["normals"], _d); r.max_distance = _p(keep["max_distance"], _d); r.min_distance = _p(keep["min_distance"], _d)
    return r, keep


def covis_desc(n_views, lists, queries, query_self=None, eligible=None, min_weight=15, max_out=None):
    """n_views, lists: one sequence of view indices per map point (its observers), queries: one sequence of point indices per
    keyframe or frame (its map points, slot order), query_self (Q,) the queries' own views (-1: a frame) or None, eligible (V,)
    or None, max_out: entries of the ordered list per query (None: n_views, the full counter) -> (movba_covis_desc, the arrays it
    points into)."""
    lists = [np.asarray(l, np.int32).reshape(-1) for l in lists]
    queries = [np.asarray(q, np.int32).reshape(-1) for q in queries]
    keep = dict(obs_ptr=np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32),
                obs_view=np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0), np.int32),
                query_ptr=np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.int32),
                query_point=np.ascontiguousarray(np.concatenate(queries) if queries else np.zeros(0), np.int32))
    d = CovisDesc()
    d.n_views, d.n_points, d.n_queries = int(n_views), len(lists), len(queries)
    d.min_weight, d.max_out = int(min_weight), int(n_views if max_out is None else max_out)
    for key in ("obs_ptr", "obs_view", "query_ptr", "query_point"):
        setattr(d, key, _p(keep[key], _i))
    if query_self is not None:
        keep["query_self"] = np.ascontiguousarray(query_self, np.int32).reshape(-1)
        if len(keep["query_self"]) != len(queries):
            raise ValueError("covis_desc: query_self has one entry per query")
        d.query_self = _p(keep["query_self"], _i)
    if eligible is not None:
        keep["eligible"] = np.ascontiguousarray(eligible, np.uint8).reshape(-1)
        if len(keep["eligible"]) != d.n_views:
            raise ValueError("covis_desc: eligible has one entry per view")
        d.eligible = _p(keep["eligible"], _u)
    return d, keep


def covis_result(n_queries, max_out, alloc=np.zeros):
    """-> (movba_covis_result with its output arrays, the arrays it points into); out_view / out_weight are (Q, max_out)"""
    keep = {key: alloc((n_queries,), np.int32) for key in COVIS_ARRAYS[:4]}
    keep["out_view"], keep["out_weight"] = alloc((n_queries, max_out), np.int32), alloc((n_queries, max_out), np.int32)
    r = CovisResult()
    for key in COVIS_ARRAYS:
        if keep[key].size or key in COVIS_ARRAYS[:4]:
            setattr(r, key, _p(keep[key], _i))
    return r, keep


def track_desc(views, queries):
    """views: one dict per view with track (n,) int32 ids in slot order and optionally taken (n,), obs (n, 2), ur (n,), depth (n,)
    (an optional array is given for every view or for none); queries: (TM_TRIANGULATION, view 1, view 2) or (TM_LOOKUP, view,
    ids) -> (movba_track_desc, the arrays it points into; keep["match_cap"]: the sum of view 1's slots over the TRIANGULATION
    queries, what the result arrays are sized to)."""
    tracks = [np.asarray(v["track"], np.int32).reshape(-1) for v in views]
    keep = dict(view_ptr=np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32),
                slot_track=np.ascontiguousarray(np.concatenate(tracks) if tracks else np.zeros(0), np.int32))
    for key, field, dtype, width in (("taken", "slot_taken", np.uint8, 1), ("obs", "slot_obs", np.float64, 2), ("ur", "slot_ur", np.float64, 1),
                                     ("depth", "slot_depth", np.float64, 1)):
        have = [key in v and v[key] is not None for v in views]
        if not any(have):
            continue
        if not all(have):
            raise ValueError(f"track_desc: {key} is given for every view or for none")
        parts = [np.asarray(v[key], dtype).reshape(len(t), width) for v, t in zip(views, tracks)]
        keep[field] = np.ascontiguousarray(np.concatenate(parts), dtype)
    modes, qviews, items, cap = [], [], [], 0
    for q in queries:
        modes.append(int(q[0]))
        if q[0] == TM_LOOKUP:
            qviews.append((-1, int(q[1])))
            items.append(np.asarray(q[2], np.int32).reshape(-1))
        else:
            qviews.append((int(q[1]), int(q[2])))
            items.append(np.zeros(0, np.int32))
            if q[0] == TM_TRIANGULATION and 0 <= int(q[1]) < len(tracks):
                cap += len(tracks[int(q[1])])
    keep["query_mode"] = np.array(modes, np.int32)
    keep["query_view"] = np.array(qviews, np.int32).reshape(len(modes), 2)
    keep["query_ptr"] = np.concatenate([[0], np.cumsum([len(i) for i in items])]).astype(np.int32)
    keep["item_track"] = np.ascontiguousarray(np.concatenate(items) if items else np.zeros(0), np.int32)
    keep["match_cap"] = cap
    d = TrackDesc()
    d.n_views, d.n_queries = len(tracks), len(modes)
    for key in ("view_ptr", "slot_track", "query_mode", "query_view", "query_ptr", "item_track"):
        setattr(d, key, _p(keep[key], _i))
    if "slot_taken" in keep:
        d.slot_taken = _p(keep["slot_taken"], _u)
    for key in ("slot_obs", "slot_ur", "slot_depth"):
        if key in keep:
            setattr(d, key, _p(keep[key], _d))
    return d, keep


def track_result(n_queries, n_items, match_cap, payload=(), alloc=np.zeros):
    """-> (movba_track_result with its output arrays, the arrays it points into); payload: which of obs1 .. depth2 to gather"""
    keep = dict(pair_ptr=alloc((n_queries + 1,), np.int32), match_slot1=alloc((match_cap,), np.int32), match_slot2=alloc((match_cap,), np.int32),
                item_slot=alloc((n_items,), np.int32), n_found=alloc((n_queries,), np.int32))
    r = TrackResult()
    for key in TRACK_INT_ARRAYS:
        setattr(r, key, _p(keep[key], _i))
    for key in payload:
        keep[key] = alloc((match_cap, 2) if key.startswith("obs") else (match_cap,), np.float64)
        setattr(r, key, _p(keep[key], _d))
    return r, keep


def express_grid(rows: int, cols: int) -> np.ndarray:
    """movba_express_grid (host only): the lattice of extract_moves over an image of rows x cols, (n, 4) int32 x y w h; the
    keypoint of a rect is (x + 8, y + 8)."""
    n = lib().movba_express_grid(rows, cols, None, 0)
    if n < 0:
        raise MovbaError(f"movba_express_grid: {status_string(n)}")
    out = np.zeros((n, 4), np.int32)
    if n and lib().movba_express_grid(rows, cols, _p(out, _i), n) != n:
        raise MovbaError("movba_express_grid: the count changed between two calls")
    return out


def express_desc(images, items, thresholds, refs=None):
    """images: one 2-D uint8 array per image (any row stride, unit column stride), or None for an image without items (it goes as
    a NULL pointer of 1 x 1); items: per image (rects (n, 4) x y w h, modes (n,) or one mode); thresholds: one per image or one
    for all; refs: None, or per image (n, 4) uint64 -> (movba_express_desc, the arrays it points into)."""
    ni = len(images)
    thresholds = np.broadcast_to(np.asarray(thresholds, np.int32), (ni,)) if ni else np.zeros(0, np.int32)
    keep = dict(images=[], rows=np.ones(ni, np.int32), cols=np.ones(ni, np.int32), stride=np.ones(ni, np.int32),
                threshold=np.array(thresholds, np.int32), image=(C.c_void_p * max(ni, 1))())
    rects, modes = [], []
    for i, (im, it) in enumerate(zip(images, items)):
        if im is not None:
            if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                raise ValueError("express_desc: an image is a 2-D uint8 array whose rows are contiguous")
            keep["images"].append(im)
            keep["image"][i] = im.ctypes.data
            keep["rows"][i], keep["cols"][i] = im.shape
            keep["stride"][i] = im.strides[0] if im.shape[0] > 1 else im.shape[1]
        r = np.asarray(it[0], np.int32).reshape(-1, 4)
        rects.append(r)
        modes.append(np.broadcast_to(np.asarray(it[1], np.int32), (len(r),)))
    keep["item_ptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rects])]).astype(np.int32)
    keep["item_rect"] = np.ascontiguousarray(np.concatenate(rects) if rects else np.zeros((0, 4)), np.int32)
    keep["item_mode"] = np.ascontiguousarray(np.concatenate(modes) if modes else np.zeros(0), np.int32)
    d = ExpressDesc()
    d.n_images = ni
    d.image = C.cast(keep["image"], C.POINTER(C.c_void_p))
    for key in ("rows", "cols", "stride", "threshold", "item_ptr", "item_rect", "item_mode"):
        setattr(d, key, _p(keep[key], _i))
    if refs is not None:
        parts = [np.asarray(r, np.uint64).reshape(-1, 4) for r in refs]
        keep["item_ref"] = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 4)), np.uint64)
        if len(keep["item_ref"]) != len(keep["item_rect"]):
            raise ValueError("express_desc: refs holds one descriptor per item")
        d.item_ref = _p(keep["item_ref"], _q)
    return d, keep


def express_result(n_items, n_images, alloc=np.zeros, distance=True):
    """-> (movba_express_result with its output arrays, the arrays it points into)"""
    keep = {key: alloc((n_items, width) if width > 1 else (n_items,), dtype) for key, dtype, width in EXPRESS_ARRAYS
            if distance or key != "distance"}
    keep["n_features"] = alloc((n_images,), np.int32)
    r = ExpressResult()
    r.code = _p(keep["code"], _u); r.desc = _p(keep["desc"], _q); r.count = _p(keep["count"], _i); r.n_features = _p(keep["n_features"], _i)
    if distance:
        r.distance = _p(keep["distance"], _i)
    return r, keep


def lattice_size(rows: int, cols: int) -> int:
    """the number of rects of movba_express_grid(rows, cols)"""
    return ((rows - 1) // 16) * ((cols - 1) // 16) if rows > 16 and cols > 16 else 0


def advance_desc(frames):
    """frames: one dict per frame with image (2-D uint8, any row stride; None for a frame without items), threshold, force_grid,
    first_id, prev_pt (n, 2), prev_mb (n, 2), prev_age, prev_track (n,), prev_desc (n, 4) uint64, prev_coverage (n,), prev_cand
    (n, 4), mv_pt (m, 2), mv_dindx (m,), kp_rect (k, 4) and grid_covered (one entry per lattice rect, or None: nothing is covered;
    when every frame says None, grid_ptr goes as NULL) -> (movba_advance_desc, the arrays it points into).  keep["n_grid"] is the
    number of lattice rects of all frames."""
    nf = len(frames)
    keep = dict(images=[], rows=np.ones(nf, np.int32), cols=np.ones(nf, np.int32), stride=np.ones(nf, np.int32),
                threshold=np.array([fr["threshold"] for fr in frames], np.int32).reshape(nf),
                force_grid=np.array([bool(fr["force_grid"]) for fr in frames], np.uint8).reshape(nf),
                first_id=np.array([fr["first_id"] for fr in frames], np.int32).reshape(nf), image=(C.c_void_p * max(nf, 1))())
    lattice = []
    for i, fr in enumerate(frames):
        im = fr["image"]
        if im is not None:
            if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                raise ValueError("advance_desc: an image is a 2-D uint8 array whose rows are contiguous")
            keep["images"].append(im)
            keep["image"][i] = im.ctypes.data
            keep["rows"][i], keep["cols"][i] = im.shape
            keep["stride"][i] = im.strides[0] if im.shape[0] > 1 else im.shape[1]
        lattice.append(lattice_size(int(keep["rows"][i]), int(keep["cols"][i])))
    keep["n_grid"] = int(sum(lattice))

    def cat(key, dtype, width):
        parts = [np.asarray(fr[key], dtype).reshape((-1, width) if width > 1 else (-1,)) for fr in frames]
        ptr = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int32)
        return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, width) if width > 1 else (0,)), dtype), ptr

    d = AdvanceDesc()
    d.n_frames = nf
    d.image = C.cast(keep["image"], C.POINTER(C.c_void_p))
    for key, dtype, width in ADVANCE_PREV:
        keep[key], ptr = cat(key, dtype, width)
        if "prev_ptr" in keep and not np.array_equal(ptr, keep["prev_ptr"]):
            raise ValueError("advance_desc: the prev_ arrays of a frame have one row per previous feature")
        keep["prev_ptr"] = ptr
    keep["mv_pt"], keep["mv_ptr"] = cat("mv_pt", np.float32, 2)
    keep["mv_dindx"], ptr = cat("mv_dindx", np.int32, 1)
    if not np.array_equal(ptr, keep["mv_ptr"]):
        raise ValueError("advance_desc: mv_pt and mv_dindx have one row per motion vector")
    keep["kp_rect"], keep["kp_ptr"] = cat("kp_rect", np.int32, 4)
    if any(fr.get("grid_covered") is not None for fr in frames):
        parts = [np.zeros(n, np.uint8) if fr.get("grid_covered") is None else np.asarray(fr["grid_covered"]).astype(bool).astype(np.uint8).reshape(-1)
                 for fr, n in zip(frames, lattice)]
        keep["grid_covered"] = np.ascontiguousarray(np.concatenate(parts), np.uint8)
        keep["grid_ptr"] = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int32)
    types = {np.dtype(np.int32): _i, np.dtype(np.uint8): _u, np.dtype(np.float32): _f, np.dtype(np.uint64): _q}
    for key, value in keep.items():
        if isinstance(value, np.ndarray):
            setattr(d, key, _p(value, types[value.dtype]))
    return d, keep


def advance_result(n_frames, n_prev, n_kps, n_grid, alloc=np.zeros):
    """-> (movba_advance_result with its output arrays, the arrays it points into)"""
    size = dict(prev=n_prev, kps=n_kps, frames=n_frames, seg=4 * n_frames + 1, cap=n_prev + n_kps + n_grid)
    types = {np.int32: _i, np.uint8: _u, np.float32: _f, np.uint64: _q}
    keep, r = {}, AdvanceResult()
    for key, dtype, width, which in ADVANCE_ARRAYS:
        keep[key] = alloc((size[which], width) if width > 1 else (size[which],), dtype)
        setattr(r, key, _p(keep[key], types[dtype]))
    return r, keep


def mv_raster_desc(frames):
    """frames: one dict per frame with rows, cols, coverage_threshold, want_grid (optional, 0), records (dict of src_x, src_y, dst_x,
    dst_y, w, h (n,) and optionally source (-1), ref (0)) and q_pt (k, 2) -> (movba_mv_raster_desc, the arrays it points into).
    keep["n_grid"] is the number of lattice rects of all frames."""
    nf = len(frames)
    keep = dict(rows=np.array([fr["rows"] for fr in frames], np.int32).reshape(nf), cols=np.array([fr["cols"] for fr in frames], np.int32).reshape(nf),
                coverage_threshold=np.array([fr["coverage_threshold"] for fr in frames], np.float64).reshape(nf),
                want_grid=np.array([bool(fr.get("want_grid", 0)) for fr in frames], np.uint8).reshape(nf))
    keep["n_grid"] = int(sum(lattice_size(int(r), int(c)) for r, c in zip(keep["rows"], keep["cols"])))
    counts = [len(np.asarray(fr["records"]["src_x"]).reshape(-1)) for fr in frames]
    keep["rec_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    for key, dtype in MV_RASTER_RECORD:
        fill = dict(source=-1, ref=0).get(key)
        parts = [np.asarray(fr["records"][key] if key in fr["records"] else np.full(n, fill), dtype).reshape(-1) for fr, n in zip(frames, counts)]
        if [len(a) for a in parts] != counts:
            raise ValueError("mv_raster_desc: the fields of a frame's records have one entry per record")
        keep[key] = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dtype)
    parts = [np.asarray(fr["q_pt"], np.float32).reshape(-1, 2) for fr in frames]
    keep["q_ptr"] = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int32)
    keep["q_pt"] = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2)), np.float32)
    d = MvRasterDesc()
    d.n_frames = nf
    types = {np.dtype(np.int32): _i, np.dtype(np.uint8): _u, np.dtype(np.float32): _f, np.dtype(np.float64): _d, np.dtype(np.int16): _h}
    for key, value in keep.items():
        if isinstance(value, np.ndarray):
            setattr(d, key, _p(value, types[value.dtype]))
    return d, keep


def mv_raster_result(n_frames, n_records, n_q, n_grid, alloc=np.zeros):
    """-> (movba_mv_raster_result with its output arrays, the arrays it points into)"""
    size = dict(ptr=n_frames + 1, rec=n_records, q=n_q, grid=n_grid, frames=n_frames)
    types = {np.int32: _i, np.uint8: _u, np.float32: _f, np.float64: _d}
    keep, r = {}, MvRasterResult()
    for key, dtype, width, which in MV_RASTER_ARRAYS:
        keep[key] = alloc((size[which], width) if width > 1 else (size[which],), dtype)
        setattr(r, key, _p(keep[key], types[dtype]))
    return r, keep


def lk_desc(frames, max_level=3, max_iter=20, eps=0.01, min_eig_threshold=1e-4):
    """frames: one dict per frame with prev and next (2-D uint8 of one shape, any row stride but the same in both; None for a
    frame without points, then with rows and cols), win and pt (n, 2) -> (movba_lk_desc, the arrays it points into)."""
    nf = len(frames)
    keep = dict(images=[], rows=np.ones(nf, np.int32), cols=np.ones(nf, np.int32), stride=np.ones(nf, np.int32),
                win=np.array([fr["win"] for fr in frames], np.int32).reshape(nf), prev_image=(C.c_void_p * max(nf, 1))(),
                next_image=(C.c_void_p * max(nf, 1))())
    for i, fr in enumerate(frames):
        a, b = fr.get("prev"), fr.get("next")
        if a is None or b is None:
            keep["rows"][i], keep["cols"][i] = fr["rows"], fr["cols"]
            keep["stride"][i] = fr["cols"]
            continue
        for im in (a, b):
            if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                raise ValueError("lk_desc: an image is a 2-D uint8 array whose rows are contiguous")
        if a.shape != b.shape or a.strides[0] != b.strides[0]:
            raise ValueError("lk_desc: the two images of a frame have one shape and one row stride")
        keep["images"] += [a, b]
        keep["prev_image"][i], keep["next_image"][i] = a.ctypes.data, b.ctypes.data
        keep["rows"][i], keep["cols"][i] = a.shape
        keep["stride"][i] = a.strides[0] if a.shape[0] > 1 else a.shape[1]
    parts = [np.asarray(fr["pt"], np.float32).reshape(-1, 2) for fr in frames]
    keep["pt_ptr"] = np.concatenate([[0], np.cumsum([len(a) for a in parts])]).astype(np.int32)
    keep["pt"] = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2)), np.float32)
    d = LkDesc()
    d.n_frames = nf
    d.prev_image = C.cast(keep["prev_image"], C.POINTER(C.c_void_p))
    d.next_image = C.cast(keep["next_image"], C.POINTER(C.c_void_p))
    for key in ("rows", "cols", "stride", "win", "pt_ptr"):
        setattr(d, key, _p(keep[key], _i))
    d.pt = _p(keep["pt"], _f)
    d.max_level, d.max_iter, d.eps, d.min_eig_threshold = max_level, max_iter, eps, min_eig_threshold
    return d, keep


def lk_result(n_frames, n_pt, alloc=np.zeros):
    """-> (movba_lk_result with its output arrays, the arrays it points into)"""
    size = dict(pt=n_pt, ptr=n_frames + 1)
    types = {np.int32: _i, np.uint8: _u, np.float32: _f}
    keep, r = {}, LkResult()
    for key, dtype, width, which in LK_ARRAYS:
        keep[key] = alloc((size[which], width) if width > 1 else (size[which],), dtype)
        setattr(r, key, _p(keep[key], types[dtype]))
    return r, keep


def stereo_desc(frames, max_row_diff=4.0, min_disparity=0.0, max_point=100):
    """frames: one dict per stereo frame with pt (n, 2), next_pt (n, 2) and pt_status (n,) - Solver.lk_track's input and output
    arrays as they are -, rows and cols (the right image's), bf, max_disparity, th_depth, cam (fx fy cx cy), select
    (STEREO_SELECT_*, default NONE) and optionally pt_un (n, 2), pose (7: Tcw) and has_point (n,).  An optional array that one frame
    has is filled in for the others with what its absence means (pt, the identity, zeros); one that no frame has is passed as
    NULL -> (movba_stereo_desc, the arrays it points into)."""
    nf = len(frames)
    parts = [np.asarray(fr["pt"], np.float32).reshape(-1, 2) for fr in frames]
    n = [len(a) for a in parts]

    def cat(key, dtype, width, default):
        for k, fr in enumerate(frames):
            if default is None and fr.get(key) is None:
                raise ValueError(f"stereo_desc: frame {k} has no {key}")
        rows = [np.asarray(fr[key], dtype).reshape((-1, width) if width > 1 else (-1,)) if fr.get(key) is not None else default(k)
                for k, fr in enumerate(frames)]
        for k, a in enumerate(rows):
            if len(a) != n[k]:
                raise ValueError(f"stereo_desc: {key} of frame {k} has {len(a)} rows for {n[k]} points")
        return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, width) if width > 1 else (0,)), dtype)

    keep = dict(pt_ptr=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
                pt=np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 2)), np.float32),
                next_pt=cat("next_pt", np.float32, 2, None), pt_status=cat("pt_status", np.uint8, 1, None))
    keep["pt_un"] = cat("pt_un", np.float32, 2, lambda k: parts[k]) if any(fr.get("pt_un") is not None for fr in frames) else None
    keep["has_point"] = (cat("has_point", np.uint8, 1, lambda k: np.zeros(n[k], np.uint8))
                         if any(fr.get("has_point") is not None for fr in frames) else None)
    identity = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    keep["poses"] = (np.ascontiguousarray([np.asarray(fr["pose"], np.float64).reshape(7) if fr.get("pose") is not None else identity
                                           for fr in frames], np.float64).reshape(nf, 7)
                     if any(fr.get("pose") is not None for fr in frames) else None)
    for key, dtype in (("rows", np.int32), ("cols", np.int32), ("bf", np.float32), ("max_disparity", np.float32), ("th_depth", np.float32)):
        keep[key] = np.array([fr[key] for fr in frames], dtype).reshape(nf)
    keep["select"] = np.array([fr.get("select", STEREO_SELECT_NONE) for fr in frames], np.int32).reshape(nf)
    keep["cam"] = np.ascontiguousarray([np.asarray(fr["cam"], np.float32).reshape(4) for fr in frames], np.float32).reshape(nf, 4)
    d = StereoDesc()
    d.n_frames = nf
    types = {np.dtype(np.int32): _i, np.dtype(np.float32): _f, np.dtype(np.uint8): _u, np.dtype(np.float64): _d}
    for key in ("pt_ptr", "pt", "next_pt", "pt_status", "pt_un", "rows", "cols", "bf", "max_disparity", "th_depth", "cam", "select", "poses",
                "has_point"):
        if keep[key] is not None:
            setattr(d, key, _p(keep[key], types[keep[key].dtype]))
    d.max_row_diff, d.min_disparity, d.max_point = max_row_diff, min_disparity, max_point
    return d, keep


def stereo_result(n_frames, n_pt, alloc=np.zeros):
    """-> (movba_stereo_result with its output arrays, the arrays it points into)"""
    size = dict(pt=n_pt, ptr=n_frames + 1, frames=n_frames)
    types = {np.int32: _i, np.uint8: _u, np.float32: _f, np.float64: _d}
    keep, r = {}, StereoResult()
    for key, dtype, width, which in STEREO_ARRAYS:
        keep[key] = alloc((size[which], width) if width > 1 else (size[which],), dtype)
        setattr(r, key, _p(keep[key], types[dtype]))
    return r, keep


def run_batch(solvers) -> int:
    """movba_lba_run_batch over the resident windows of `solvers` (created on one stream); download each as usual."""
    arr = (C.c_void_p * len(solvers))(*[s._h for s in solvers])
    rc = solvers[0]._L.movba_lba_run_batch(arr, len(solvers))
    if rc < 0:
        raise MovbaError(f"movba_lba_run_batch: {status_string(rc)}")
    return rc


class Solver:
    """One handle = one device + one stream (movba_create / movba_destroy)."""

    def __init__(self, device: int = 0, stream: int | None = None, pcg_rel_tol: float = 0.0,
                 pcg_max_iters: int = 0, run_ahead: int = 0, profile=False, pcg_coarse: bool = True, host_wait: int = 0,
                 pcg_spill: bool = False, direct: bool = False, reorder: bool = True, solver: int | None = None, hooks: bool = False):
        self._h = C.c_void_p()
        self._L = lib(hooks)                # (hooks: the test build, whose handles take movba_test_hook)
        self._hooks = hooks
        self._pinned_blocks = []
        opt = Options(pcg_rel_tol, pcg_max_iters, run_ahead, (0x3f if profile is True else int(profile)), 0 if pcg_coarse else -1, host_wait, 1 if pcg_spill else 0, (int(solver) if solver is not None else (1 if direct else 0)), 0 if reorder else -1, 0)
        rc = self._L.movba_create(C.byref(self._h), device, C.c_void_p(stream) if stream else None, C.byref(opt))
        if rc != OK:
            self._h = C.c_void_p()
            raise MovbaError(f"movba_create failed: {status_string(rc)} (no CPU fallback)")
        self._keep = None

    def hook(self, name: str, value: int):
        """movba_test_hook (test build only: Solver(hooks=True)): host_structure, entries_unpacked, no_sorted_structure,
        pcg_packed, helper_delay_us, wait_ticks, band_park_trial, device_cus set a switch and return 0; batch_variant sets
        nothing and returns what the last movba_lba_run_batch over this handle launched with (decode with batch_variant())"""
        if not self._hooks:
            raise MovbaError("test hooks exist in libmovba_hooks.so only: Solver(hooks=True)")
        rc = self._L.movba_test_hook(self._h, name.encode(), int(value))
        if rc < 0:
            raise MovbaError(f"movba_test_hook({name}): {status_string(rc)}")
        return rc

    def batch_variant(self) -> dict:
        """The record of the last batched run (test build only): the kernel variant every batched launch took - ldsp, overflow,
        padded, stereo: the fold over the batch's windows -, the number of stream groups, and where this window ran."""
        v = self.hook("batch_variant", 0)
        return dict(ldsp=v & 1, overflow=(v >> 1) & 1, padded=(v >> 2) & 1, stereo=(v >> 3) & 1, groups=(v >> 4) & 15,
                    batched=(v >> 8) & 1, solo=(v >> 9) & 1)

    def stamp_records(self, cls: int):
        """movba_stamp_records (clock-stamp build only, -DMOVBA_CLOCK_STAMP; not in include/movba.h): the records the last run left,
        (n, 8) uint64; cls 0: back-substitution pass per workgroup, 1: k_schur per wave, 2: the segment slots"""
        if not hasattr(self._L, "movba_stamp_records"):
            raise MovbaError("movba_stamp_records exists in the clock-stamp build only (MOVBA_LIB)")
        f = self._L.movba_stamp_records
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = f(self._h, cls, None, 0)
        if n < 0:
            raise MovbaError(f"movba_stamp_records: {status_string(n)}")
        a = np.zeros((n, 8), np.uint64)
        if f(self._h, cls, a.ctypes.data, n) != n:
            raise MovbaError("movba_stamp_records: the record count changed between two calls")
        return a

    def close(self):
        if self._h:
            self._L.movba_destroy(self._h)
            self._h = C.c_void_p()
        if getattr(self, "_pinned_blocks", None):
            self._prep = None
            for p in self._pinned_blocks:
                self._L.movba_host_free(p)
            self._pinned_blocks = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- results ---------------------------------------------------------------
    def _pinned(self, shape, dtype=np.float64):
        """array in movba_host_alloc memory (released by close()); float64 unless said otherwise"""
        n = int(np.prod(shape))
        item = np.dtype(dtype).itemsize
        p = self._L.movba_host_alloc(max(item * n, 8))
        if not p:
            raise MovbaError("movba_host_alloc failed")
        self._pinned_blocks.append(p)
        a = np.frombuffer((C.c_uint8 * max(item * n, 8)).from_address(p), dtype=dtype, count=n).reshape(shape)
        a[...] = 0
        return a

    def _pin_inputs(self, d, keep):
        """The descriptor's input arrays moved into movba_host_alloc memory (what a C++ caller that flattens its window into
        buffers of the library's allocator hands over: the adapter's): the device reads the index arrays where they lie and the
        copy engine takes the observations and estimates straight out of them, nothing is staged."""
        for key, field, ptr in (("poses", "poses", _d), ("fixed", "pose_fixed", _u), ("points", "points", _d), ("ep", "edge_pose", _i),
                                ("el", "edge_point", _i), ("obs", "obs", _d), ("isg", "inv_sigma2", _d), ("obs_right", "obs_right", _d)):
            if key not in keep:
                continue
            a = self._pinned(keep[key].shape, keep[key].dtype)
            a[...] = keep[key]
            keep[key] = a
            setattr(d, field, _p(a, ptr))

    def _alloc_result(self, d, pinned=False, chi2=True):
        mk = self._pinned if pinned else np.zeros
        out = dict(poses=mk((d.n_poses, 7)), points=mk((d.n_points, 3)),
                   chi2=mk((d.n_edges,)) if chi2 else np.zeros(0), outlier=np.zeros(d.n_edges, np.uint8))
        r = LbaResult()
        r.poses = _p(out["poses"], _d); r.points = _p(out["points"], _d)
        if chi2:
            r.chi2 = _p(out["chi2"], _d)                  # (left NULL: the per-edge chi2 is neither exported nor copied out)
        r.outlier = _p(out["outlier"], _u)
        return r, out

    @staticmethod
    def _pack(r, out, rc):
        n = r.n_trace
        out.update(status=rc, iters_done=r.iters_done, n_solves=r.n_solves, n_outliers=r.n_outliers,
                   pcg_iters=r.pcg_iters, last_rejected=r.last_rejected, lam=r.lambda_, cost0=r.cost0, cost=r.cost,
                   n_direct=r.n_direct, direct_from=r.direct_from, n_chol_fail=r.n_chol_fail, n_pcg_giveups=r.n_pcg_giveups,
                   n_sync_timeouts=r.n_sync_timeouts, n_band=r.n_band,
                   trace=dict(lam=np.array(r.tr_lambda[:n]), f0=np.array(r.tr_f0[:n]), f1=np.array(r.tr_f1[:n]),
                              rho=np.array(r.tr_rho[:n]), accept=np.array(r.tr_accept[:n]),
                              pcg=np.array(r.tr_pcg_iters[:n])))
        return out

    def solve(self, w, flags=FLAG_STALE_ERROR_QUIRK, stop=None, max_iters=None, max_trials=0) -> dict:
        d, keep = make_desc(w, flags, stop, max_iters, max_trials)
        r, out = self._alloc_result(d)
        rc = self._L.movba_lba_solve(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_lba_solve: {status_string(rc)}")
        self._keep = (d, keep)             # (download() may be called again on the solved window)
        if rc != OK:                       # silent early return: nothing written, echo the inputs
            out["poses"][:] = keep["poses"]; out["points"][:] = keep["points"]
        return self._pack(r, out, rc)

    def prepare(self, w, flags=FLAG_STALE_ERROR_QUIRK, stop=None, max_iters=None, max_trials=0, pinned=False, chi2=True):
        """Descriptor and result buffers built once for repeated solve_prepared() calls: what a C++ caller that keeps its
        flattened arrays and result buffers does (nothing is allocated or converted per call).  pinned=True: the buffers are
        blocks of movba_host_alloc memory that live until close() (results handed out earlier stay valid): prepare a window
        once and keep it - `self._prep` may be saved and put back to alternate between prepared windows - rather than
        preparing it again for every call."""
        d, keep = make_desc(w, flags, stop, max_iters, max_trials)
        if pinned:
            self._pin_inputs(d, keep)                     # ... and input arrays the device reads where they lie
        r, out = self._alloc_result(d, pinned, chi2)      # pinned: result arrays the solve's last kernel writes into directly
        self._keep = (d, keep)
        self._prep = (d, keep, r, out)

    def solve_prepared(self, pack=True):
        """movba_lba_solve on the prepared buffers; pack=False returns only the status (results stay in the buffers)."""
        d, keep, r, out = self._prep
        rc = self._L.movba_lba_solve(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_lba_solve: {status_string(rc)}")
        if not pack:
            return rc
        if rc != OK:
            out["poses"][:] = keep["poses"]; out["points"][:] = keep["points"]
        return self._pack(r, dict(out), rc)

    def upload_prepared(self):
        """movba_lba_upload of the prepared descriptor (phased calls on buffers built once: batched runs)"""
        d, keep, r, out = self._prep
        rc = self._L.movba_lba_upload(self._h, C.byref(d))
        if rc < 0:
            raise MovbaError(f"movba_lba_upload: {status_string(rc)}")
        self._keep = (d, keep)
        return rc

    def download_prepared(self, pack=False):
        """movba_lba_download into the prepared result buffers"""
        d, keep, r, out = self._prep
        rc = self._L.movba_lba_download(self._h, C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_lba_download: {status_string(rc)}")
        return self._pack(r, dict(out), rc) if pack else rc

    def upload(self, w, flags=FLAG_STALE_ERROR_QUIRK, stop=None, max_iters=None, max_trials=0):
        d, keep = make_desc(w, flags, stop, max_iters, max_trials)
        rc = self._L.movba_lba_upload(self._h, C.byref(d))
        if rc < 0:
            raise MovbaError(f"movba_lba_upload: {status_string(rc)}")
        self._keep = (d, keep)
        return rc

    def run(self) -> int:
        rc = self._L.movba_lba_run(self._h)
        if rc < 0:
            raise MovbaError(f"movba_lba_run: {status_string(rc)}")
        return rc

    def download(self) -> dict:
        d, keep = self._keep
        r, out = self._alloc_result(d)
        rc = self._L.movba_lba_download(self._h, C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_lba_download: {status_string(rc)}")
        if rc != OK:
            out["poses"][:] = keep["poses"]; out["points"][:] = keep["points"]
        return self._pack(r, out, rc)

    def marginals(self, damping: float = 0.0, points: bool = True, pose_cov=None, point_cov=None) -> dict:
        """movba_lba_marginals on the window of the last run: dict(status, pose_cov (NP, 6, 6), point_cov (P, 3, 3) or None).
        status OK or SINGULAR (nothing written: the arrays come back as they were - NaN unless given); errors raise.
        pose_cov / point_cov: C-contiguous float64 arrays of those shapes to write into (allocated when not given)."""
        d, keep = self._keep
        if pose_cov is None:
            pose_cov = np.full((d.n_poses, 6, 6), np.nan)
        if points and point_cov is None:
            point_cov = np.full((d.n_points, 3, 3), np.nan)
        for a, shape in ((pose_cov, (d.n_poses, 6, 6)), (point_cov if points else None, (d.n_points, 3, 3))):
            if a is not None and (a.shape != shape or a.dtype != np.float64 or not a.flags.c_contiguous):
                raise ValueError(f"marginals: output arrays must be C-contiguous float64 of shape {shape}")
        rc = self._L.movba_lba_marginals(self._h, float(damping), _p(pose_cov, _d), _p(point_cov, _d) if points else None)
        if rc < 0:
            raise MovbaError(f"movba_lba_marginals: {status_string(rc)}")
        return dict(status=rc, pose_cov=pose_cov, point_cov=point_cov if points else None)

    def export_poses_device(self, dst_ptr: int, nbytes: int):
        rc = self._L.movba_lba_export_poses_device(self._h, C.c_void_p(dst_ptr), nbytes)
        if rc != OK:
            raise MovbaError(f"movba_lba_export_poses_device: {status_string(rc)}")

    def set_pose_export(self, dst_ptr: int, nbytes: int):
        """Register a device buffer that every later run() leaves the optimised poses in (0 unregisters)."""
        rc = self._L.movba_lba_set_pose_export(self._h, C.c_void_p(dst_ptr) if dst_ptr else None, nbytes)
        if rc != OK:
            raise MovbaError(f"movba_lba_set_pose_export: {status_string(rc)}")

    def profile(self) -> dict:
        p = Profile()
        self._L.movba_get_profile(self._h, C.byref(p))
        return dict(kernels={p.name[k].decode(): dict(ms=p.ms[k], launches=p.launches[k]) for k in range(NKERNELS)},
                    upload_ms=p.upload_ms, structure_ms=p.structure_ms, download_ms=p.download_ms)

    def reset_profile(self):
        self._L.movba_reset_profile(self._h)

    def set_profile_mask(self, mask: int):
        self._L.movba_set_profile_mask(self._h, mask)

    def pose_opt(self, Xw, obs, pose0, cam, huber_delta, chi2_gate, rounds=4, its=10, inv_sigma2=None, ransac_iters=0, ransac_seed=1,
                 confidence=0.0, lo_iters=0) -> dict:
        d, r, keep = _pose_desc(Xw, obs, pose0, cam, huber_delta, chi2_gate, rounds, its, inv_sigma2, ransac_iters, ransac_seed,
                                confidence, lo_iters)
        rc = self._L.movba_pose_opt(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_pose_opt: {status_string(rc)}")
        return _pose_dict(r, keep, rc)

    def pose_opt_batch(self, frames) -> list:
        """movba_pose_opt_batch: `frames` is a list of dicts with pose_opt's keyword arguments (Xw, obs, pose0, cam,
        huber_delta, chi2_gate, optional rounds, its, inv_sigma2, ransac_iters, ransac_seed, confidence, lo_iters); one dict per
        frame back, pose_opt's keys with the frame's own status (0, or 3 = MOVBA_EMPTY for fewer than 4 matches)."""
        n = len(frames)
        descs = (PoseDesc * max(n, 1))(); res = (PoseResult * max(n, 1))()
        keeps = []
        for k, f in enumerate(frames):
            d, r, keep = _pose_desc(**f)
            descs[k] = d; res[k] = r
            keeps.append(keep)
        rc = self._L.movba_pose_opt_batch(self._h, descs, res, n)
        if rc < 0:
            raise MovbaError(f"movba_pose_opt_batch: {status_string(rc)}")
        return [_pose_dict(res[k], keeps[k], res[k].status) for k in range(n)]

    def triangulate(self, views, pairs, matches, reproj_gate=5.0, far_threshold=0.0, pinned=False, points=None, code=None) -> dict:
        """movba_triangulate (the numeric body of LocalMapping::CreateNewMapPoints): views dict(poses, cam, optional bf, b),
        pairs dict(pair_view, pair_ptr), matches dict(obs1, obs2, optional ur1, ur2, depth1, depth2) ->
        dict(points (M, 3), code (M,) uint8 TRI_*, n_accepted, status).  pinned: result arrays in movba_host_alloc memory
        (written by the kernel itself; they live until close()); points / code: arrays to write into instead."""
        d, keep = tri_desc(views, pairs, matches, reproj_gate, far_threshold)
        n = int(keep["pair_ptr"][-1]) if "pair_ptr" in keep and len(keep["pair_ptr"]) else 0
        if points is None:
            points = self._pinned((n, 3)) if pinned else np.zeros((n, 3))
        if code is None:
            code = self._pinned((n,), np.uint8) if pinned else np.zeros(n, np.uint8)
        r = TriResult()
        r.points = _p(points, _d); r.code = _p(code, _u)
        rc = self._L.movba_triangulate(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_triangulate: {status_string(rc)}")
        return dict(points=points, code=code, n_accepted=r.n_accepted, status=rc)

    def _pair_alloc(self, pinned, k):
        """(alloc, alloc_by) of pair k's result arrays for two_view_desc / init_map_desc: pinned is one flag for every array
        of every pair, or a sequence with one set of array names per pair."""
        if np.isscalar(pinned):
            return (self._pinned if pinned else np.zeros), None
        return np.zeros, {name: self._pinned for name in pinned[k]}

    def two_view(self, pairs, pinned=False, diagnostics=False, lo_iters=None) -> list:
        """movba_two_view (monocular map initialisation, TwoViewReconstruction::Reconstruct) on a list of frame pairs:
        dicts with obs1, obs2 (M, 2) pixels, cam (fx, fy, cx, cy) and optionally the keys of TWO_VIEW_DEFAULTS.  One dict per
        pair back: status (0, or 3 = MOVBA_EMPTY under 5 matches), outcome (TV_*), pose (T21), E (3, 3), parallax_deg,
        n_inliers, n_pass, n_good, samples_used, inlier, points, good, code (TV_CHK_*) per match and, with diagnostics,
        hyp_nsol, hyp_E, hyp_loss.  pinned: per-match arrays in movba_host_alloc memory (written by the kernels; they live
        until close()) - True / False for all of them, or a sequence with one set of array names per pair.  lo_iters: None
        calls movba_two_view; an integer calls movba_two_view_lo (local optimisation of the winner with that many steps at
        most) and adds lo_kept, lo_steps, loss0, loss, n_inliers0 and E0 (3, 3) to every dict."""
        n = len(pairs)
        descs = (TwoViewDesc * max(n, 1))(); res = (TwoViewResult * max(n, 1))()
        keeps = []
        for k, pair in enumerate(pairs):
            alloc, by = self._pair_alloc(pinned, k)
            d, r, keep = two_view_desc(pair, alloc, diagnostics, alloc_by=by)
            descs[k] = d; res[k] = r
            keeps.append(keep)
        if lo_iters is None:
            rc = self._L.movba_two_view(self._h, descs, res, n)
        else:
            info = (TwoViewLoInfo * max(n, 1))()
            rc = self._L.movba_two_view_lo(self._h, descs, res, n, int(lo_iters), info)
        if rc < 0:
            raise MovbaError(f"movba_two_view{'' if lo_iters is None else '_lo'}: {status_string(rc)}")
        out = []
        for k in range(n):
            r, keep = res[k], keeps[k]
            o = dict(status=r.status, outcome=r.outcome, pose=np.array(r.pose[:]), E=np.array(r.E[:]).reshape(3, 3),
                     parallax_deg=r.parallax_deg, n_inliers=r.n_inliers, n_pass=r.n_pass, n_good=r.n_good,
                     samples_used=r.samples_used)
            o.update({key: keep[key] for key in ("inlier", "points", "good", "code", "hyp_nsol", "hyp_E", "hyp_loss") if key in keep})
            if lo_iters is not None:
                fo = info[k]
                o.update(lo_kept=fo.kept, lo_steps=fo.steps, loss0=fo.loss0, loss=fo.loss, n_inliers0=fo.n_inliers0,
                         E0=np.array(fo.E0[:]).reshape(3, 3))
            out.append(o)
        return out

    def init_map(self, pairs, pinned=False, trace=False) -> list:
        """movba_init_map (the two-keyframe bundle adjustment, median depth and rescaling of
        Tracking::CreateInitialMapMonocular) on a list of frame pairs: dicts as init_map_desc takes them - movba_two_view's
        pose, points and good go in as pose2, points and use.  One dict per pair back: status (0, or 3 = MOVBA_EMPTY without
        a used match), outcome (IM_*), pose (T21), points (M, 3), chi2 (M, 2), median_depth, n_used, iters_done, n_solves,
        last_rejected, n_chol_fail, lam, cost0, cost and, with trace, trace = dict(lam, f0, f1, rho, accept).  pinned:
        per-match arrays in movba_host_alloc memory (written by the kernel; they live until close()) - as two_view.  A pair
        with chi2=False leaves chi2 out (None comes back)."""
        n = len(pairs)
        descs = (InitMapDesc * max(n, 1))(); res = (InitMapResult * max(n, 1))()
        tr = (InitMapTrace * max(n, 1))() if trace else None
        keeps = []
        for k, pair in enumerate(pairs):
            alloc, by = self._pair_alloc(pinned, k)
            d, r, keep = init_map_desc(pair, alloc, pair.get("chi2", True), alloc_by=by)
            descs[k] = d; res[k] = r
            keeps.append(keep)
        rc = self._L.movba_init_map(self._h, descs, res, n, tr)
        if rc < 0:
            raise MovbaError(f"movba_init_map: {status_string(rc)}")
        out = []
        for k in range(n):
            r, keep = res[k], keeps[k]
            o = dict(status=r.status, outcome=r.outcome, pose=np.array(r.pose[:]), points=keep["points"], chi2=keep.get("chi2"),
                     median_depth=r.median_depth, n_used=r.n_used, iters_done=r.iters_done, n_solves=r.n_solves,
                     last_rejected=r.last_rejected, n_chol_fail=r.n_chol_fail, lam=r.lambda_, cost0=r.cost0, cost=r.cost)
            if trace:
                t, nt = tr[k], tr[k].n_trace
                o["trace"] = dict(lam=np.array(t.tr_lambda[:nt]), f0=np.array(t.tr_f0[:nt]), f1=np.array(t.tr_f1[:nt]),
                                  rho=np.array(t.tr_rho[:nt]), accept=np.array(t.tr_accept[:nt]))
            out.append(o)
        return out

    def view_points(self, points, views, pinned=False, arrays=tuple(VIEW_ITEM_ARRAYS)) -> dict:
        """movba_view_points (Frame::isInFrustum, the gates at the head of MOVMatcher::Fuse, KeyFrame::ComputeSceneMedianDepth):
        points dict(points (N, 3), normals (N, 3), max_distance, min_distance (N,) - the last three only when a view is not a
        DEPTH view), views a list of dicts with mode (VIEW_*), pose (7,), cam (fx, fy, cx, cy), items (indices into the point
        table) and optionally bf, bounds (minX, maxX, minY, maxY), log_scale_factor, n_levels, cos_limit, q ->
        dict(status, view_ptr, code (uint8 VP_*) and the per-item arrays named in `arrays` (z, uv, dist, view_cos, level, ur,
        track_depth) over all views' items in view order, n_accepted and median_depth per view).  pinned: result arrays in
        movba_host_alloc memory (written by the kernels themselves; they live until close())."""
        d, keep = view_desc(points, views)
        r, out = view_result(len(keep["item_point"]), len(views), self._pinned if pinned else np.zeros, arrays)
        rc = self._L.movba_view_points(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_view_points: {status_string(rc)}")
        out.update(status=rc, view_ptr=keep["view_ptr"])
        return out

    def point_normals(self, points, views, lists, ref_view, ref_level, scale_factors, pinned=False) -> dict:
        """movba_point_normals (the numeric body of MapPoint::UpdateNormalAndDepth): points (N, 3), views (V, 7) poses Tcw,
        lists: one sequence of view indices per point (its observers, in the order they are summed), ref_view (N,) the
        reference keyframe as a view index, ref_level (N,) the keypoint's octave there, scale_factors (L,) ->
        dict(status, normals (N, 3), max_distance, min_distance (N,)): what view_points takes under those names; NaN for a
        point without observers.  pinned: result arrays in movba_host_alloc memory (written by the kernel itself; they live
        until close())."""
        d, keep = normals_desc(points, views, lists, ref_view, ref_level, scale_factors)
        r, out = normals_result(d.n_points, self._pinned if pinned else np.zeros)
        rc = self._L.movba_point_normals(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_point_normals: {status_string(rc)}")
        out.update(status=rc)
        return out

    def covisibility(self, n_views, lists, queries, query_self=None, eligible=None, min_weight=15, max_out=None, pinned=False) -> dict:
        """movba_covisibility (the count, threshold, maximum and ordering of KeyFrame::UpdateConnections and of the voting loop
        of Tracking::UpdateLocalKeyFrames): arguments as covis_desc -> dict(status, n_counted, n_connected, best_view,
        best_weight (Q,), out_view, out_weight (Q, max_out)): per query its counted views by weight descending, ties by view
        index descending, padded with -1 / 0.  pinned: result arrays in movba_host_alloc memory, written by the kernel itself."""
        d, keep = covis_desc(n_views, lists, queries, query_self, eligible, min_weight, max_out)
        r, out = covis_result(d.n_queries, d.max_out, self._pinned if pinned else np.zeros)
        rc = self._L.movba_covisibility(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_covisibility: {status_string(rc)}")
        out["status"] = rc
        return out

    def track_match(self, views, queries, pinned=False) -> dict:
        """movba_track_match (the track-id joins of MOVMatcher): arguments as track_desc -> dict(status, n_matches, pair_ptr, pairs =
        dict(pair_view, pair_ptr), matches = dict(obs1, obs2, ur1, ur2, depth1, depth2: those whose source the views carry),
        match_slot1, match_slot2 (match_cap,), item_slot (n_items,), query_ptr, n_found).  `pairs` and `matches` are what
        Solver.triangulate takes, unchanged, when every query of the call is a TRIANGULATION query (a LOOKUP query stands in
        pair_view with view 1 = -1).  pinned: result arrays in movba_host_alloc memory, written by the kernels themselves."""
        d, keep = track_desc(views, queries)
        payload = [key for key, src in TRACK_PAYLOAD if "slot_" + src in keep]
        r, out = track_result(d.n_queries, len(keep["item_track"]), keep["match_cap"], payload, self._pinned if pinned else np.zeros)
        rc = self._L.movba_track_match(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_track_match: {status_string(rc)}")
        return dict(status=rc, n_matches=r.n_matches, pair_ptr=out["pair_ptr"], pairs=dict(pair_view=keep["query_view"], pair_ptr=out["pair_ptr"]),
                    matches={key: out[key] for key in payload}, match_slot1=out["match_slot1"], match_slot2=out["match_slot2"],
                    item_slot=out["item_slot"], query_ptr=keep["query_ptr"], n_found=out["n_found"])

    def express(self, images, items, thresholds, refs=None, pinned=False) -> dict:
        """movba_express (EXPRESS detection and descriptors, the pixel arithmetic of MOVExtractor): arguments as express_desc
        -> dict(status, code (n,) uint8, desc (n, 4) uint64, count, distance (n,), n_features (n_images,), item_ptr).  pinned:
        result arrays in movba_host_alloc memory, written by the kernels themselves."""
        d, keep = express_desc(images, items, thresholds, refs)
        r, out = express_result(len(keep["item_rect"]), d.n_images, self._pinned if pinned else np.zeros)
        rc = self._L.movba_express(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_express: {status_string(rc)}")
        out.update(status=rc, item_ptr=keep["item_ptr"])
        return out

    def advance(self, frames, pinned=False) -> dict:
        """movba_advance (the inter-frame walk of MOVExtractor: sort, vector choice, claims, gate, new macroblocks, grid, track
        ids): frames as advance_desc -> dict(status, order, fate, chosen_mv, distance (n_prev,), kp_found, kp_code (n_kps,),
        mov_cnt, grid_ran, next_id (n_frames,), seg_ptr (4 n_frames + 1,), feat_src, feat_track, feat_pt, feat_rect, feat_age,
        feat_desc (capacity rows, padded behind seg_ptr[-1]), prev_ptr, kp_ptr).  pinned: result arrays in movba_host_alloc
        memory, written by the kernels themselves."""
        d, keep = advance_desc(frames)
        r, out = advance_result(d.n_frames, len(keep["prev_age"]), len(keep["kp_rect"]), keep["n_grid"], self._pinned if pinned else np.zeros)
        rc = self._L.movba_advance(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_advance: {status_string(rc)}")
        out.update(status=rc, prev_ptr=keep["prev_ptr"], kp_ptr=keep["kp_ptr"])
        return out

    def mv_raster(self, frames, pinned=False) -> dict:
        """movba_mv_raster (the decoder's motion-vector image, VideoDecoder::NextImage's loop over the records, read at the query
        points and never formed): frames as mv_raster_desc -> dict(status, kept_ptr, grid_ptr (n_frames + 1,), kp_rect, mv_pt,
        mv_dindx (n_records rows, padded behind kept_ptr[-1]), rec_kept (n_records,), cand (n_q, 4), grid_covered (n_grid,),
        cover_px, coverage_area, force_grid (n_frames,), rec_ptr, q_ptr).  kept_ptr, kp_rect, mv_pt, mv_dindx, cand, grid_covered
        and force_grid are what advance_desc takes (kept_ptr as mv_ptr and kp_ptr, cand as prev_cand).  pinned: result arrays in
        movba_host_alloc memory, written by the kernels themselves."""
        d, keep = mv_raster_desc(frames)
        r, out = mv_raster_result(d.n_frames, len(keep["src_x"]), len(keep["q_pt"]), keep["n_grid"], self._pinned if pinned else np.zeros)
        rc = self._L.movba_mv_raster(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_mv_raster: {status_string(rc)}")
        out.update(status=rc, rec_ptr=keep["rec_ptr"], q_ptr=keep["q_ptr"])
        return out

    def lk_track(self, frames, max_level=3, max_iter=20, eps=0.01, min_eig_threshold=1e-4, pinned=False) -> dict:
        """movba_lk_track (sparse pyramidal Lucas-Kanade, cv::calcOpticalFlowPyrLK as the reference calls it, for the points of
        many frames): frames as lk_desc -> dict(status, next_pt (n_pt, 2), pt_status, err, exit_code, keep (n_pt,), kept_ptr
        (n_frames + 1,), kept_src (n_pt, padded with -1 behind kept_ptr[-1]), pt_ptr).  The defaults are the reference's.
        pinned: result arrays in movba_host_alloc memory, written by the kernels themselves."""
        d, keep = lk_desc(frames, max_level, max_iter, eps, min_eig_threshold)
        r, out = lk_result(d.n_frames, len(keep["pt"]), self._pinned if pinned else np.zeros)
        rc = self._L.movba_lk_track(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_lk_track: {status_string(rc)}")
        out.update(status=rc, pt_ptr=keep["pt_ptr"])
        return out

    def stereo_points(self, frames, max_row_diff=4.0, min_disparity=0.0, max_point=100, pinned=False) -> dict:
        """movba_stereo_points (the stereo gates behind the left-to-right LK call, the median-distance pruning, the un-projection
        and the choice of new map points, for the keypoints of many frames): frames as stereo_desc - they take lk_track's pt,
        next_pt and pt_status as they are -> dict(status, u_right, depth, code (n_pt,), n_stereo, median_dist, th_dist
        (n_frames,), sel_ptr (n_frames + 1,), sel_src, sel_new (n_pt, padded with -1 / 0 behind sel_ptr[-1]), sel_cam, sel_point
        (n_pt, 3, padded with NaN), pt_ptr).  u_right and depth are what lba obs_right and triangulate's ur1 / depth1 take.  The
        defaults are the reference's.  pinned: result arrays in movba_host_alloc memory, written by the kernels themselves."""
        d, keep = stereo_desc(frames, max_row_diff, min_disparity, max_point)
        r, out = stereo_result(d.n_frames, len(keep["pt"]), self._pinned if pinned else np.zeros)
        rc = self._L.movba_stereo_points(self._h, C.byref(d), C.byref(r))
        if rc < 0:
            raise MovbaError(f"movba_stereo_points: {status_string(rc)}")
        out.update(status=rc, pt_ptr=keep["pt_ptr"])
        return out

    def lba_point_normals(self, ref_pose, ref_level, scale_factors, outlier=None, pinned=False) -> dict:
        """movba_lba_point_normals: the same quantities for every map point of the window of the last run, read where it lies
        on the device.  ref_pose (P,) indexes the window's poses, ref_level (P,), scale_factors (L,); outlier: (E,) flags in
        caller edge order (what download returned) whose edges are skipped, or None -> dict(status, normals (P, 3),
        max_distance, min_distance (P,)).  pinned: as point_normals."""
        d, keep = self._keep
        ref_pose = np.ascontiguousarray(ref_pose, np.int32).reshape(-1)
        ref_level = np.ascontiguousarray(ref_level, np.int32).reshape(-1)
        scale = np.ascontiguousarray(scale_factors, np.float64).reshape(-1)
        if len(ref_pose) != d.n_points or len(ref_level) != d.n_points:
            raise ValueError("lba_point_normals: ref_pose and ref_level have one entry per map point of the window")
        if outlier is not None:
            outlier = np.ascontiguousarray(outlier, np.uint8).reshape(-1)
            if len(outlier) != d.n_edges:
                raise ValueError("lba_point_normals: outlier has one entry per edge of the window")
        r, out = normals_result(d.n_points, self._pinned if pinned else np.zeros)
        rc = self._L.movba_lba_point_normals(self._h, _p(ref_pose, _i), _p(ref_level, _i), _p(scale, _d), len(scale),
                                             _p(outlier, _u) if outlier is not None else None, r.normals, r.max_distance, r.min_distance)
        if rc < 0:
            raise MovbaError(f"movba_lba_point_normals: {status_string(rc)}")
        out.update(status=rc)
        return out
