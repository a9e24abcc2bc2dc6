"""ctypes binding of the C ABI in include/msfm_match.h (libmsfm_match.so, built in-tree).

There is no fallback: if the shared library is missing or no gfx950 GPU is usable, loading /
context creation raises.  Nothing here imports the CPU oracle.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmsfm_match.so")
if os.environ.get("MSFM_LIBRARY"):   # development hook: an alternative build of the same C ABI (tools/variant_bench.sh)
    LIB_PATH = os.path.abspath(os.environ["MSFM_LIBRARY"])

OK, E_INVALID, E_DEVICE, E_NOIMAGE, E_CAPACITY, E_STATE = range(6)
DTYPE_F32, DTYPE_U8 = 0, 1
ORDER_SSE4X4, ORDER_AVX2_FMA, ORDER_AVX512_FMA = 0, 1, 3
MAX_IMAGES = 10000
DIM = 128

VERIFY_FUNDAMENTAL, VERIFY_ESSENTIAL, VERIFY_HOMOGRAPHY = 0, 1, 2


class TwoViewParams(C.Structure):
    _fields_ = [("min_num_inliers", C.c_int32), ("reserved", C.c_int32), ("tri_max_error", C.c_double), ("tri_min_angle", C.c_double)]


# msfm_two_view_record (include/msfm_match.h): 144 bytes, no implicit padding
TWO_VIEW_RECORD = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_kept", "<i4"),
                            ("n_positive_depth", "<i4"), ("n_triangulated", "<i4"), ("is_initial_candidate", "<i4"),
                            ("median_tri_angle", "<f8"), ("mean_tri_angle", "<f8"), ("mean_residual", "<f8")])


class TwoViewRefineParams(C.Structure):
    _fields_ = [("max_iters", C.c_int32), ("min_matches", C.c_int32), ("step_tol", C.c_double)]


# msfm_two_view_refinement (include/msfm_match.h): 40 bytes, no implicit padding; its status bits
TWO_VIEW_REFINEMENT = np.dtype([("status", "<i4"), ("stop", "<i4"), ("steps", "<i4"), ("accepted", "<i4"),
                                ("n_positive_depth_before", "<i4"), ("n_triangulated_before", "<i4"), ("cost_before", "<f8"),
                                ("cost_after", "<f8")])
TVR_ELIGIBLE, TVR_STEP_ACCEPTED, TVR_REFINED = 1, 2, 4


def two_view_refined(refinements):
    """The pairs whose two-view record was replaced by its refined one: a bool mask over a TWO_VIEW_REFINEMENT array."""
    return (np.asarray(refinements)["status"] & TVR_REFINED) != 0


class TrackParams(C.Structure):
    _fields_ = [("min_pair_matches", C.c_int32), ("add_only", C.c_int32)]


class TrackFilter(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("max_length", C.c_int32), ("keep_inconsistent", C.c_int32), ("reserved", C.c_int32)]


class TrackStats(C.Structure):
    """msfm_track_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("nodes", "edges", "pairs", "pairs_skipped", "pairs_below_min", "matches_ignored", "tracks_total",
                                         "tracks_inconsistent", "tracks_over_max_length", "tracks_kept", "observations_kept",
                                         "longest_track", "device_bytes")] + [("fold_ms", C.c_double), ("finish_ms", C.c_double)]


# track triangulation (include/msfm_match.h): status bits, the 104-byte pose, the 48-byte record
TRI_ATTEMPTED, TRI_POINT, TRI_ERROR_OK, TRI_ANGLE_OK, TRI_DEPTH_OK = 1, 2, 4, 8, 16
POSE_RT = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,))])
POINT3D = np.dtype([("status", "<i4"), ("n_views", "<i4"), ("X", "<f8", (3,)), ("mean_residual", "<f8"), ("tri_angle", "<f8")])


class TriangulationParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("min_angle", C.c_double), ("min_views", C.c_int32), ("reserved", C.c_int32)]


class TriangulationStats(C.Structure):
    """msfm_triangulation_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("tracks", "attempted", "with_point", "error_ok", "angle_ok", "depth_ok", "succeeded",
                                         "observations_used", "device_bytes")] + [("triangulate_ms", C.c_double)]


# robust track triangulation (include/msfm_match.h): the record's extra status bit, the 24-byte parameters, the 40-byte stats
TRI_ROBUST = 32


class RobustTriangulationParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("min_angle", C.c_double), ("min_views", C.c_int32), ("max_hypotheses", C.c_int32)]


class RobustStats(C.Structure):
    """msfm_robust_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("retried", "rescued", "observations_rejected", "hypotheses")] + [("robust_ms", C.c_double)]


# point refinement (include/msfm_match.h): the record's extra status bit, the 16-byte parameters, the 72-byte stats
TRI_REFINED = 64


class RefineParams(C.Structure):
    _fields_ = [("step_tol", C.c_double), ("max_iters", C.c_int32), ("reserved", C.c_int32)]


class RefineStats(C.Structure):
    """msfm_refine_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("eligible", "refined", "gained_error_ok", "rejected_by_verdict", "iterations")] + \
               [(k, C.c_double) for k in ("cost_before", "cost_after", "refine_ms", "prepare_ms")]


def refined(points):
    """The records of a POINT3D array whose point is a refined one (MSFM_TRI_REFINED)."""
    return (np.asarray(points)["status"] & TRI_REFINED) != 0


# pose refinement (include/msfm_match.h): the record's extra status bit, the 16-byte parameters, the 104-byte stats, the 48-byte record
TRI_REPOSED = 128
POSE_ATTEMPTED, POSE_REFINED, POSE_FIXED = 1, 2, 4
POSE_REFINEMENT = np.dtype([("image_id", "<i4"), ("status", "<i4"), ("n_observations", "<i4"), ("iterations", "<i4"), ("stop", "<i4"),
                            ("inliers_before", "<i4"), ("inliers_after", "<i4"), ("reserved", "<i4"), ("cost_before", "<f8"),
                            ("cost_after", "<f8")])


class PoseRefineParams(C.Structure):
    _fields_ = [("step_tol", C.c_double), ("max_iters", C.c_int32), ("min_observations", C.c_int32)]


class PoseRefineStats(C.Structure):
    """msfm_pose_refine_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("images", "eligible", "refined", "rejected_by_inliers", "iterations", "observations",
                                         "points_reposed", "points_lost", "points_gained")] + \
               [(k, C.c_double) for k in ("cost_before", "cost_after", "refine_ms", "prepare_ms")]


def reposed(points):
    """The records of a POINT3D array that a pose refinement evaluated again under changed poses (MSFM_TRI_REPOSED)."""
    return (np.asarray(points)["status"] & TRI_REPOSED) != 0


# map extension (include/msfm_match.h): the record's extra status bit, the 8-byte parameters, the 96-byte stats
TRI_EXTENDED = 256


class ExtendParams(C.Structure):
    _fields_ = [("max_hypotheses", C.c_int32), ("reserved", C.c_int32)]


class ExtendStats(C.Structure):
    """msfm_extend_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("images_added", "tracks_touched", "continued", "observations_added", "observations_rejected",
                                         "created_attempted", "created", "retried", "succeeded", "observations_used")] + \
               [(k, C.c_double) for k in ("extend_ms", "prepare_ms")]


def extended(points):
    """The records of a POINT3D array that a map extension continued into new images or created (MSFM_TRI_EXTENDED)."""
    return (np.asarray(points)["status"] & TRI_EXTENDED) != 0


# map filtering (include/msfm_match.h): the record's extra status bit, the 16-byte parameters, the 88-byte stats
TRI_FILTERED = 512


class FilterParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("min_angle", C.c_double)]


class FilterStats(C.Structure):
    """msfm_filter_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("eligible", "dropped_by_depth", "dropped_by_error", "trimmed", "regained", "removed_by_views",
                                         "removed_by_angle", "succeeded", "observations_used")] + \
               [(k, C.c_double) for k in ("filter_ms", "prepare_ms")]


def filtered(points):
    """The records of a POINT3D array that a map filtering trimmed or removed (MSFM_TRI_FILTERED)."""
    return (np.asarray(points)["status"] & TRI_FILTERED) != 0


# map completion (include/msfm_match.h): the record's extra status bit, the 8-byte parameters, the 80-byte stats
TRI_COMPLETED = 1024


class CompleteParams(C.Structure):
    _fields_ = [("max_error", C.c_double)]


class CompleteStats(C.Structure):
    """msfm_complete_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("eligible", "candidates", "admitted", "rejected_by_depth", "rejected_by_error", "completed",
                                         "succeeded", "observations_used")] + \
               [(k, C.c_double) for k in ("complete_ms", "prepare_ms")]


def completed(points):
    """The records of a POINT3D array that a map completion admitted an observation into (MSFM_TRI_COMPLETED)."""
    return (np.asarray(points)["status"] & TRI_COMPLETED) != 0


# map visibility (include/msfm_match.h): bases, routes, record flags, the 8-byte parameters, the 24-byte record, the 56-byte stats
VIS_TRACKS, VIS_MAP = 0, 1
VIS_ROUTE_AUTO, VIS_ROUTE_GLOBAL, VIS_ROUTE_LDS = 0, 1, 2
VIS_POSED, VIS_QUERIED = 1, 2
VISIBILITY = np.dtype([(k, "<i4") for k in ("image_id", "flags", "n_elements", "n_visible", "n_points", "reserved")])
_VIS_BASES = {"tracks": VIS_TRACKS, "map": VIS_MAP}
_VIS_ROUTES = {"auto": VIS_ROUTE_AUTO, "global": VIS_ROUTE_GLOBAL, "lds": VIS_ROUTE_LDS}


class VisibilityParams(C.Structure):
    _fields_ = [("basis", C.c_int32), ("route", C.c_int32)]


class VisibilityStats(C.Structure):
    """msfm_visibility_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("tracks_counted", "elements_counted", "pair_increments", "device_bytes")] + \
               [(k, C.c_int32) for k in ("images", "posed", "query", "route")] + [("visibility_ms", C.c_double)]


def _by_count(ids, counts):
    """ids by count descending, id ascending -> list of int"""
    ids, counts = np.asarray(ids, np.int64), np.asarray(counts, np.int64)
    return [int(i) for i in ids[np.lexsort((ids, -counts))]]


def next_images(records, min_visible=15):
    """Map::GetNextImageIds over Context.visibility()'s records: the images without a pose that see at least min_visible standing
    points (15: register_images' min_inliers), by n_visible descending, id ascending."""
    r = np.asarray(records)
    r = r[((r["flags"] & VIS_POSED) == 0) & (r["n_visible"] >= int(min_visible))]
    return _by_count(r["image_id"], r["n_visible"])


def local_window(row, records, image_id, size=5):
    """Map::GetLocalBAData over one row of Context.visibility()'s matrix (the row of image_id): the posed images other than image_id
    that share a point with it, by shared count descending, id ascending, at most `size` (the reference's kMaxRelatedImageNum = 5)."""
    r, row = np.asarray(records), np.asarray(row)
    keep = ((r["flags"] & VIS_POSED) != 0) & (r["image_id"] != int(image_id)) & (row > 0)
    return _by_count(r["image_id"][keep], row[keep])[:max(int(size), 0)]


def initial_first_images(records):
    """FindFirstInitialImage's order over Context.visibility(basis="tracks")'s records: every image by n_elements descending, id
    ascending."""
    r = np.asarray(records)
    return _by_count(r["image_id"], r["n_elements"])


def initial_second_images(row, records, image_id):
    """FindSecondInitialImage's order over the row of image_id: the other images by shared count descending, id ascending, images that
    share nothing left out."""
    r, row = np.asarray(records), np.asarray(row)
    keep = (r["image_id"] != int(image_id)) & (row > 0)
    return _by_count(r["image_id"][keep], row[keep])


# map alignment (include/msfm_match.h): the record's extra status bit, the estimate's status bits, the per-prior flags, the 104-byte
# similarity, the 24-byte parameters, the 144-byte record, the 16-byte per-prior record, the 48-byte stats
TRI_ALIGNED = 4096
ALN_ATTEMPTED, ALN_MODEL, ALN_SUCCEEDED, ALN_REFIT, ALN_LEAST_SQUARES = 1, 2, 4, 8, 16
ALN_USED, ALN_INLIER = 1, 2
ALIGNMENT_RESIDUAL = np.dtype([("flags", "<i4"), ("reserved", "<i4"), ("error", "<f8")])


class Similarity(C.Structure):
    """msfm_similarity: world' = s Q X + d, Q row-major."""
    _fields_ = [("s", C.c_double), ("Q", C.c_double * 9), ("d", C.c_double * 3)]


class AlignmentParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("confidence", C.c_double), ("max_hypotheses", C.c_int32), ("min_inliers", C.c_int32)]


class Alignment(C.Structure):
    """msfm_alignment (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int32) for k in ("status", "n_listed", "n_used", "n_inliers", "hypotheses", "refits")] + \
               [("similarity", Similarity), ("rms", C.c_double), ("estimate_ms", C.c_double)]


class TransformStats(C.Structure):
    """msfm_transform_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("poses_transformed", "points_transformed", "points_lost", "points_gained", "succeeded")] + \
               [("transform_ms", C.c_double)]


def similarity_struct(s, Q, d):
    """(s, Q 3 x 3, d 3) -> Similarity"""
    return Similarity(float(s), (C.c_double * 9)(*np.asarray(Q, np.float64).reshape(9)), (C.c_double * 3)(*np.asarray(d, np.float64).reshape(3)))


def alignment_dict(a):
    """An Alignment struct -> dict: its integers, rms, estimate_ms, and the similarity as s (float), Q (3 x 3), d (3)."""
    out = {k: getattr(a, k) for k, _ in Alignment._fields_ if k != "similarity"}
    out.update(s=float(a.similarity.s), Q=np.array(a.similarity.Q, np.float64).reshape(3, 3), d=np.array(a.similarity.d, np.float64))
    return out


def prior_table(positions):
    """{image id: (x, y, z)} -> (ids int32 by ascending id, positions float64 [n, 3])"""
    ids = np.asarray(sorted(int(i) for i in positions), np.int32)
    pos = np.zeros((max(len(ids), 1), 3), np.float64)
    for k, i in enumerate(ids):
        pos[k] = np.asarray(positions[int(i)], np.float64).reshape(3)
    return ids, pos[:len(ids)]


def aligned(points):
    """The records of a POINT3D array that the last transform_map moved (MSFM_TRI_ALIGNED) and that no later call has rewritten: every
    call that rewrites a record clears the bit."""
    return (np.asarray(points)["status"] & TRI_ALIGNED) != 0


def succeeded(points):
    """The reference's is_succeed per record of a POINT3D array: POINT & ERROR_OK & ANGLE_OK."""
    want = TRI_POINT | TRI_ERROR_OK | TRI_ANGLE_OK
    return (np.asarray(points)["status"] & want) == want


# image registration (include/msfm_match.h): status bits, the 128-byte record
REG_ATTEMPTED, REG_POSE, REG_SUCCEEDED, REG_REFINED = 1, 2, 4, 8
REGISTRATION = np.dtype([("image_id", "<i4"), ("status", "<i4"), ("n_correspondences", "<i4"), ("n_inliers", "<i4"), ("hypotheses", "<i4"),
                         ("reserved", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("mean_residual", "<f8")])


class RegisterParams(C.Structure):
    _fields_ = [("max_error", C.c_double), ("confidence", C.c_double), ("max_iters", C.c_int32), ("min_inliers", C.c_int32),
                ("refine_iters", C.c_int32), ("reserved", C.c_int32)]


class RegisterStats(C.Structure):
    """msfm_register_stats (include/msfm_match.h)."""
    _fields_ = [("images", C.c_int32), ("attempted", C.c_int32), ("succeeded", C.c_int32), ("rounds", C.c_int32),
                ("correspondences", C.c_int64), ("hypotheses", C.c_int64), ("device_bytes", C.c_int64), ("register_ms", C.c_double)]


def registered(records):
    """The reference's is_succeed per record of a REGISTRATION array: the SUCCEEDED bit."""
    return (np.asarray(records)["status"] & REG_SUCCEEDED) != 0


def registered_poses(records, poses=None):
    """The succeeded records as the dict image id -> (R, t) that triangulate_tracks takes, merged over `poses` (which is not changed)."""
    out = dict(poses) if poses else {}
    for r in np.asarray(records)[registered(records)]:
        out[int(r["image_id"])] = (r["R"].reshape(3, 3).copy(), r["t"].copy())
    return out


def camera_struct(camera):
    """A dict or sequence fx, fy, cx, cy[, k1, k2, p1, p2] (missing distortion coefficients are 0) -> Camera."""
    keys = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")
    vals = [camera.get(k, 0.0) for k in keys] if isinstance(camera, dict) else list(camera) + [0.0] * (8 - len(camera))
    return Camera(*[float(v) for v in vals[:8]])


def pose_table(poses):
    """dict image id -> (R 3 x 3, t 3) [or None: listed but not valid] -> (ids int32, POSE_RT array), by ascending id.  A pair (ids,
    POSE_RT array), the form Context.pose_list() returns, is passed on IN THE GIVEN ORDER (a copy; the C API takes the list in any
    order)."""
    if not isinstance(poses, dict):
        ids, tab = poses
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        tab = np.array(tab, POSE_RT).reshape(-1)
        if len(ids) != len(tab):
            raise ValueError("pose list: %d ids for %d poses" % (len(ids), len(tab)))
        return ids, tab
    ids = np.asarray(sorted(int(i) for i in poses), np.int32)
    tab = np.zeros(max(len(ids), 1), POSE_RT)
    for k, i in enumerate(ids):
        if poses[int(i)] is None:
            continue
        R, t = poses[int(i)]
        tab[k]["valid"] = 1
        tab[k]["R"] = np.asarray(R, np.float64).reshape(9)
        tab[k]["t"] = np.asarray(t, np.float64).reshape(3)
    return ids, tab[:len(ids)]


class MatchParams(C.Structure):
    _fields_ = [("ratio", C.c_float), ("cross_check", C.c_int), ("max_distance", C.c_double)]


class Camera(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]


# camera refinement (include/msfm_match.h): the record's extra status bit, the unknowns' bits, the 24-byte parameters, the 248-byte stats
TRI_RECALIBRATED = 2048
CAM_FX_FY, CAM_F, CAM_CX_CY, CAM_K1_K2 = 1, 2, 4, 8
_CAM_BITS = {"fx_fy": CAM_FX_FY, "f": CAM_F, "cx_cy": CAM_CX_CY, "k1_k2": CAM_K1_K2}


class CameraRefineParams(C.Structure):
    _fields_ = [("step_tol", C.c_double), ("mask", C.c_int32), ("max_iters", C.c_int32), ("min_observations", C.c_int32),
                ("reserved", C.c_int32)]


class CameraRefineStats(C.Structure):
    """msfm_camera_refine_stats (include/msfm_match.h)."""
    _fields_ = [(k, C.c_int64) for k in ("observations", "behind", "iterations", "accepted_steps", "stop", "refined", "rejected_by_inliers",
                                         "inliers_before", "inliers_after", "points_recalibrated", "points_lost", "points_gained")] + \
               [("cost_before", C.c_double), ("cost_after", C.c_double), ("camera_before", Camera), ("camera_after", Camera),
                ("refine_ms", C.c_double)]


def camera_dict(cam):
    """A Camera struct -> {"fx": .., "fy": .., "cx": .., "cy": .., "k1": .., "k2": .., "p1": .., "p2": ..}"""
    return {k: float(getattr(cam, k)) for k, _ in Camera._fields_}


def camera_mask(mask):
    """MSFM_CAM_* bits from an int or from names out of "fx_fy", "f", "cx_cy", "k1_k2" (one name or a sequence of them)."""
    if isinstance(mask, (int, np.integer)):
        return int(mask)
    bits = 0
    for name in ((mask,) if isinstance(mask, str) else mask):
        bits |= _CAM_BITS[name]
    return bits


def recalibrated(points):
    """The records of a POINT3D array that a camera refinement evaluated again under the new camera (MSFM_TRI_RECALIBRATED) and that
    no refine_points, refine_poses, filter_points or complete_points has rewritten since: those clear the bit on what they rewrite."""
    return (np.asarray(points)["status"] & TRI_RECALIBRATED) != 0


class VerifyParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("max_iters", C.c_int), ("seed", C.c_ulonglong)]


class Profile(C.Structure):
    _fields_ = [("dist_kernel_ms", C.c_double), ("dist_kernel_launches", C.c_int),
                ("total_device_ms", C.c_double), ("descriptor_pairs", C.c_int64),
                ("dist_algo_bytes", C.c_int64), ("approx_kernel_ms", C.c_double),
                ("approx_kernel_launches", C.c_int), ("prefilter_pairs", C.c_int), ("fallback_pairs", C.c_int),
                ("candidates", C.c_int64), ("prefilter_descriptor_pairs", C.c_int64),
                ("exact_descriptor_pairs", C.c_int64), ("tie_rows", C.c_int64),
                ("sweep2_ms", C.c_double), ("sweep2_launches", C.c_int), ("compacted_pairs", C.c_int),
                ("sweep2_descriptor_pairs", C.c_int64), ("verify_ms", C.c_double),
                ("sub_batches", C.c_int), ("tie_queue_regrows", C.c_int), ("plan_regrows", C.c_int),
                ("sweep1_i8_launches", C.c_int), ("sweep1_q8_launches", C.c_int), ("sweep1b_launches", C.c_int),
                ("sweep1b_ms", C.c_double), ("sweep1b_descriptor_pairs", C.c_int64), ("order_sensitive_rows", C.c_int64),
                ("demoted_pairs", C.c_int), ("mixed_route_sub_batches", C.c_int), ("memory_shrinks", C.c_int)]


class Chunk(C.Structure):
    """msfm_chunk: one completed device sub-batch of a streaming series (msfm_match_pairs_begin / _next)."""
    _fields_ = [("first_pair", C.c_int), ("n_pairs", C.c_int), ("count", C.c_int64), ("offsets", C.POINTER(C.c_int64)),
                ("qt", C.POINTER(C.c_int32)), ("dist", C.POINTER(C.c_float)), ("d_qt", C.c_void_p), ("d_dist", C.c_void_p),
                ("sensitive_rows", C.POINTER(C.c_int32))]


class Memory(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("device_free", "device_total", "store", "inbox", "scratch", "results_device", "page_locked_host")]


class RetrievalParams(C.Structure):
    _fields_ = [("num_words", C.c_int), ("train_iters", C.c_int), ("train_rows", C.c_int64)]


class RetrievalProfile(C.Structure):
    _fields_ = [("train_ms", C.c_double), ("train_iterations", C.c_int), ("assign_ms", C.c_double), ("score_ms", C.c_double),
                ("topk_ms", C.c_double), ("rows", C.c_int64), ("num_words", C.c_int)]


class MsfmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("msfm error %d: %s" % (code, msg))
        self.code = code


def _signatures():
    """The C surface of include/msfm_match.h: name -> (restype, argtypes).  load() applies it; EXPORTS is its list of names."""
    P, i, i64, vp = C.POINTER, C.c_int, C.c_int64, C.c_void_p
    ip, fp, i64p, u8p, intp = P(C.c_int32), P(C.c_float), P(i64), P(C.c_uint8), P(i)
    mp, cam = P(MatchParams), P(Camera)
    return {
        "msfm_version": (C.c_char_p, []),
        "msfm_device_count": (i, []),
        "msfm_create": (i, [i, P(vp)]),
        "msfm_destroy": (None, [vp]),
        "msfm_last_error": (C.c_char_p, [vp]),
        "msfm_device_info": (i, [vp, C.c_char_p, i, intp, intp]),
        "msfm_set_accum_order": (i, [vp, i]),
        "msfm_set_prefilter": (i, [vp, i]),
        "msfm_get_profile": (i, [vp, P(Profile)]),
        "msfm_set_limits": (i, [vp, i, i64]),
        "msfm_set_pipeline": (i, [vp, i]),
        "msfm_upload_image": (i, [vp, i, vp, i, i, i]),
        "msfm_image_rows": (i, [vp, i, intp]),
        "msfm_subset_image": (i, [vp, i, i, ip, i]),
        "msfm_clear_images": (i, [vp]),
        "msfm_finalize_store": (i, [vp]),
        "msfm_store_info": (i, [vp, i64p, i64p, i64p]),
        "msfm_upload_keypoints": (i, [vp, i, fp, i, i]),
        "msfm_match_pair": (i, [vp, i, i, C.c_float, i, C.c_double, ip, fp, intp]),
        "msfm_match_pairs": (i, [vp, ip, i, mp, i64p]),
        "msfm_match_pairs_verified": (i, [vp, ip, i, mp, P(VerifyParams), i64p]),
        "msfm_match_pairs_begin": (i, [vp, ip, i, mp, i, P(VerifyParams)]),
        "msfm_match_pairs_next": (i, [vp, P(Chunk)]),
        "msfm_match_pairs_end": (i, [vp]),
        "msfm_fetch_matches": (i, [vp, ip, fp]),
        "msfm_view_matches": (i, [vp, P(ip), P(fp), i64p]),
        "msfm_fetch_matches_device": (i, [vp, vp, vp]),
        "msfm_fetch_order_certificate": (i, [vp, ip]),
        "msfm_read_device": (i, [vp, vp, vp, i64]),
        "msfm_memory_info": (i, [vp, P(Memory)]),
        "msfm_knn2_pair": (i, [vp, i, i, ip, fp, fp, ip, fp, fp]),
        "msfm_topscale_select": (i, [fp, i, i, ip, intp]),
        "msfm_pair_id": (i, [i, i, ip]),
        "msfm_pair_from_id": (i, [C.c_int32, intp, intp]),
        "msfm_swap_image_pair": (i, [i, i]),
        # vocabulary retrieval (matching mode 2)
        "msfm_train_vocabulary": (i, [vp, ip, i, P(RetrievalParams), u8p, intp]),
        "msfm_set_vocabulary": (i, [vp, u8p, i]),
        "msfm_image_words": (i, [vp, i, ip]),
        "msfm_retrieve_pairs": (i, [vp, ip, i, i, ip, fp, intp, fp]),
        "msfm_get_retrieval_profile": (i, [vp, P(RetrievalProfile)]),
        # geometric verification
        "msfm_set_verification_model": (i, [vp, i, cam]),
        "msfm_get_verification_stats": (i, [vp, i64p, intp]),
        "msfm_set_model_selection": (i, [vp, i, C.c_double]),
        "msfm_fetch_model_selection": (i, [vp, ip, ip, ip]),
        "msfm_set_two_view_geometry": (i, [vp, i, P(TwoViewParams)]),
        "msfm_fetch_two_view_geometry": (i, [vp, vp]),
        "msfm_set_two_view_refinement": (i, [vp, i, P(TwoViewRefineParams)]),
        "msfm_fetch_two_view_refinements": (i, [vp, vp]),
        # feature tracks and the reconstruction stage
        "msfm_tracks_begin": (i, [vp, ip, i, P(TrackParams)]),
        "msfm_tracks_add": (i, [vp, ip, i, i64p, ip]),
        "msfm_tracks_export_forest": (i, [vp, ip]),
        "msfm_tracks_import_forest": (i, [vp, ip]),
        "msfm_tracks_finish": (i, [vp, P(TrackFilter), P(TrackStats)]),
        "msfm_fetch_tracks": (i, [vp, i64p, ip, ip, u8p]),
        "msfm_fetch_track_ids": (i, [vp, i, ip]),
        "msfm_tracks_end": (i, [vp]),
        "msfm_triangulate_tracks": (i, [vp, cam, ip, vp, i, P(TriangulationParams), P(TriangulationStats)]),
        "msfm_fetch_points3d": (i, [vp, vp, P(C.c_double)]),
        "msfm_triangulate_tracks_robust": (i, [vp, cam, ip, vp, i, P(RobustTriangulationParams), P(TriangulationStats), P(RobustStats)]),
        "msfm_fetch_point_inliers": (i, [vp, vp]),
        "msfm_refine_points": (i, [vp, P(RefineParams), P(RefineStats)]),
        "msfm_refine_poses": (i, [vp, P(PoseRefineParams), ip, i, P(PoseRefineStats)]),
        "msfm_fetch_poses": (i, [vp, ip, vp, intp]),
        "msfm_fetch_pose_refinements": (i, [vp, vp]),
        "msfm_refine_camera": (i, [vp, P(CameraRefineParams), P(CameraRefineStats)]),
        "msfm_fetch_camera": (i, [vp, cam]),
        "msfm_extend_points": (i, [vp, ip, vp, i, P(ExtendParams), P(ExtendStats)]),
        "msfm_filter_points": (i, [vp, P(FilterParams), ip, i, P(FilterStats)]),
        "msfm_complete_points": (i, [vp, P(CompleteParams), ip, i, P(CompleteStats)]),
        "msfm_map_visibility": (i, [vp, P(VisibilityParams), ip, i, vp, vp, P(VisibilityStats)]),
        "msfm_estimate_alignment": (i, [vp, ip, P(C.c_double), i, P(AlignmentParams), P(Alignment), vp]),
        "msfm_transform_map": (i, [vp, P(Similarity), P(TransformStats)]),
        "msfm_register_images": (i, [vp, cam, ip, i, P(RegisterParams), P(RegisterStats)]),
        "msfm_fetch_registrations": (i, [vp, vp, vp, vp, vp, vp]),
    }


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)
_lib = None


def load():
    """Load libmsfm_match.so; raises (loudly) if the HIP extension has not been built or lacks a declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C monocularsfm_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)   # raises AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _dict(st):
    """A ctypes stats struct as a dict of its fields."""
    return {k: getattr(st, k) for k, _ in st._fields_}


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Context:
    """One matcher context bound to one GPU (msfm_ctx)."""

    def __init__(self, device=0, order=ORDER_SSE4X4):
        # PyTorch-ROCm bundles a HIP runtime of its own (torch/lib/libamdhip64.so) next to the system one this library links: two
        # runtimes in one process.  Measured on the GPU box: torch's cannot find a device any more once the system runtime has been
        # initialised first ("No HIP GPUs are available"), the other order works.  So when torch is already imported and has not
        # touched the GPU yet, let it do so before msfm_create (bench.py / sharding.py set their device before creating a context).
        import sys
        torch = sys.modules.get("torch")
        if torch is not None:
            try:
                if torch.cuda.is_available() and not torch.cuda.is_initialized():
                    torch.cuda.init()
            except Exception:   # noqa: BLE001  (no GPU for torch: msfm_create below reports the real state)
                pass
        self._L = load()
        h = C.c_void_p()
        rc = self._L.msfm_create(int(device), C.byref(h))
        if rc != OK:
            raise MsfmError(rc, "msfm_create(device=%d) failed: no usable gfx950 GPU (there is no CPU fallback)" % device)
        self._h = h
        self.device = int(device)
        if order != ORDER_SSE4X4:
            self.set_accum_order(order)

    def close(self):
        if getattr(self, "_h", None):
            self._L.msfm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != OK:
            raise MsfmError(rc, self._L.msfm_last_error(self._h).decode())

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mhz = C.c_int(), C.c_int()
        self._chk(self._L.msfm_device_info(self._h, name, 256, C.byref(cu), C.byref(mhz)))
        return {"name": name.value.decode(), "cu_count": cu.value, "clock_mhz": mhz.value}

    def set_accum_order(self, order):
        self._chk(self._L.msfm_set_accum_order(self._h, int(order)))

    def set_prefilter(self, enable):
        """True / 1 (default): MFMA prefilter + exact re-check (byte images on the integer matrix cores); 2: fp16 matrix
        cores only; False / 0: brute-force exact kernel only."""
        self._chk(self._L.msfm_set_prefilter(self._h, 2 if enable == 2 and enable is not True else int(bool(enable))))

    def set_limits(self, max_pairs_per_batch=0, scratch_bytes=0):
        """Sub-batch limits of match_pairs (<= 0: default).  Results do not depend on them."""
        self._chk(self._L.msfm_set_limits(self._h, int(max_pairs_per_batch), int(scratch_bytes)))

    def set_pipeline(self, min_sub_batches=0):
        """A large call is cut into at least this many (shrinking) sub-batches whose tails overlap the next ones' sweeps (<= 0:
        default 2; 1: off).  Results do not depend on it."""
        self._chk(self._L.msfm_set_pipeline(self._h, int(min_sub_batches)))

    def profile(self):
        p = Profile()
        self._chk(self._L.msfm_get_profile(self._h, C.byref(p)))
        return _dict(p)

    def upload_image(self, image_id, desc):
        desc = np.asarray(desc)
        if desc.dtype == np.uint8:
            dtype = DTYPE_U8
        else:
            desc = desc.astype(np.float32, copy=False)
            dtype = DTYPE_F32
        desc = np.ascontiguousarray(desc)
        if desc.ndim != 2:
            raise ValueError("descriptors must be 2-D")
        n, dim = desc.shape
        if n == 0:
            dim = DIM
        self._chk(self._L.msfm_upload_image(self._h, int(image_id), desc.ctypes.data_as(C.c_void_p), n, dim, dtype))

    def subset_image(self, src_id, dst_id, rows):
        """dst = the given rows of the resident image src (device-side gather; no host descriptors needed)."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._chk(self._L.msfm_subset_image(self._h, int(src_id), int(dst_id), _ip(rows), len(rows)))

    def image_rows(self, image_id):
        n = C.c_int()
        self._chk(self._L.msfm_image_rows(self._h, int(image_id), C.byref(n)))
        return n.value

    def clear_images(self):
        self._chk(self._L.msfm_clear_images(self._h))

    def finalize_store(self):
        """Build everything uploaded so far now (otherwise the first matching call does it)."""
        self._chk(self._L.msfm_finalize_store(self._h))

    def store_info(self):
        """-> {device_bytes, rows, pending_images} of the descriptor store."""
        b, r, p = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.msfm_store_info(self._h, C.byref(b), C.byref(r), C.byref(p)))
        return {"device_bytes": b.value, "rows": r.value, "pending_images": p.value}

    # ---- vocabulary retrieval (matching mode 2; include/msfm_match.h) ----
    def train_vocabulary(self, ids, num_words=0, train_iters=0, train_rows=0):
        """Train the flat vocabulary on the images `ids` and keep it resident -> the words (V' x 128 uint8)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        prm = RetrievalParams(int(num_words), int(train_iters), int(train_rows))
        cap = int(num_words) if num_words else 16384
        out = np.zeros((cap, DIM), np.uint8)
        nw = C.c_int()
        self._chk(self._L.msfm_train_vocabulary(self._h, _ip(ids), len(ids), C.byref(prm), out.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(nw)))
        return out[:nw.value].copy()

    def set_vocabulary(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint8).reshape(-1, DIM)
        self._chk(self._L.msfm_set_vocabulary(self._h, words.ctypes.data_as(C.POINTER(C.c_uint8)), len(words)))

    def image_words(self, image_id):
        """The nearest word of every row of one resident image (int32)."""
        out = np.zeros(max(1, self.image_rows(image_id)), np.int32)
        self._chk(self._L.msfm_image_words(self._h, int(image_id), _ip(out)))
        return out[:self.image_rows(image_id)]

    def retrieve_pairs(self, ids, num_nearest=50, score_matrix=False):
        """-> (pairs P x 2 int32 (id1 > id2, brute mode's order), scores P float32[, n x n scores in the order of ids])."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        pairs = np.zeros((max(1, n * int(num_nearest)), 2), np.int32)
        scores = np.zeros(len(pairs), np.float32)
        mat = np.zeros((n, n), np.float32) if score_matrix else None
        cnt = C.c_int()
        self._chk(self._L.msfm_retrieve_pairs(self._h, _ip(ids), n, int(num_nearest), _ip(pairs), _fp(scores), C.byref(cnt),
                                              _fp(mat) if mat is not None else None))
        k = cnt.value
        if score_matrix:
            return pairs[:k].copy(), scores[:k].copy(), mat
        return pairs[:k].copy(), scores[:k].copy()

    def retrieval_profile(self):
        p = RetrievalProfile()
        self._chk(self._L.msfm_get_retrieval_profile(self._h, C.byref(p)))
        return _dict(p)

    def match_pair(self, id1, id2, ratio=0.8, cross_check=True, max_distance=0.7):
        n1 = max(self.image_rows(id1), 1)
        qt = np.empty((n1, 2), np.int32)
        d = np.empty(n1, np.float32)
        cnt = C.c_int()
        self._chk(self._L.msfm_match_pair(self._h, int(id1), int(id2), C.c_float(ratio), int(bool(cross_check)),
                                          float(max_distance), _ip(qt), _fp(d), C.byref(cnt)))
        m = cnt.value
        return qt[:m, 0].copy(), qt[:m, 1].copy(), d[:m].copy()

    def _view(self):
        """(qt[M,2], dist[M]) as NumPy views of the context's result buffers: no copy, valid until the next
        matching call on this context."""
        qp, dp, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_float)(), C.c_int64()
        self._chk(self._L.msfm_view_matches(self._h, C.byref(qp), C.byref(dp), C.byref(n)))
        M = n.value
        if M == 0:
            return np.zeros((0, 2), np.int32), np.zeros(0, np.float32)
        return np.ctypeslib.as_array(qp, shape=(M, 2)), np.ctypeslib.as_array(dp, shape=(M,))

    def _match(self, pairs, prm, vprm, fetch):
        """The blocking call: msfm_match_pairs, or msfm_match_pairs_verified under the VerifyParams vprm."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        P = pairs.shape[0]
        offs = np.zeros(P + 1, np.int64)
        o = offs.ctypes.data_as(C.POINTER(C.c_int64))
        if vprm is None:
            self._chk(self._L.msfm_match_pairs(self._h, _ip(pairs), P, C.byref(prm), o))
        else:
            self._chk(self._L.msfm_match_pairs_verified(self._h, _ip(pairs), P, C.byref(prm), C.byref(vprm), o))
        if not fetch:
            return offs, None, None
        if fetch == "view":
            return (offs,) + self._view()
        M = int(offs[-1])
        qt = np.empty((max(M, 1), 2), np.int32)
        d = np.empty(max(M, 1), np.float32)
        self._chk(self._L.msfm_fetch_matches(self._h, _ip(qt), _fp(d)))
        return offs, qt[:M], d[:M]

    def match_pairs(self, pairs, ratio=0.8, cross_check=True, max_distance=0.7, fetch=True):
        """pairs: P x 2 int array -> (offsets[P+1], qt[M,2], dist[M]); fetch=False skips the copy-out,
        fetch="view" returns views of the context's buffers (valid until the next matching call)."""
        return self._match(pairs, MatchParams(ratio, int(bool(cross_check)), max_distance), None, fetch)

    def match_pairs_stream(self, pairs, ratio=0.8, cross_check=True, max_distance=0.7, verified=False, copy=True, verify=None):
        """Generator over the device sub-batches of the job, in pair order (msfm_match_pairs_begin / _next): nothing accumulates in the
        library.  Yields dicts {first, n_pairs, offsets[n+1] (relative to the chunk), qt[m, 2], dist[m], sensitive[n], d_qt, d_dist
        (device pointers)}; with copy=False qt / dist / offsets are views, valid until the next item is requested.  verify: None (the
        reference's constants) or a dict of match_pairs_verified's threshold, confidence, max_iters, seed.  A context has one series
        at a time: beginning another one (or any other matching call) ends this one, whose next item is then an E_STATE error."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        prm = MatchParams(ratio, int(bool(cross_check)), max_distance)
        vprm = None
        if verify is not None:
            v = dict(dict(threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed), **verify)
            vprm = VerifyParams(v["threshold"], v["confidence"], int(v["max_iters"]), int(v["seed"]))
        self._chk(self._L.msfm_match_pairs_begin(self._h, _ip(pairs), pairs.shape[0], C.byref(prm), int(bool(verified)),
                                                 C.byref(vprm) if vprm is not None else None))
        # the library keeps ONE series per context and cannot tell whose it is: the context counts them, and a generator whose series
        # a newer one has superseded neither reads the newer one's chunks nor ends it
        self._series = mine = getattr(self, "_series", 0) + 1
        ch = Chunk()
        done = False
        try:
            while True:
                if self._series != mine:
                    raise MsfmError(E_STATE, "this series was superseded by a newer one on the same context")
                self._chk(self._L.msfm_match_pairs_next(self._h, C.byref(ch)))
                n = ch.n_pairs
                if n == 0:
                    done = True
                    return
                m = int(ch.count)
                offs = np.ctypeslib.as_array(ch.offsets, shape=(n + 1,))
                qt = np.ctypeslib.as_array(ch.qt, shape=(m, 2)) if m else np.zeros((0, 2), np.int32)
                d = np.ctypeslib.as_array(ch.dist, shape=(m,)) if m else np.zeros(0, np.float32)
                sens = np.ctypeslib.as_array(ch.sensitive_rows, shape=(n,))
                if copy:
                    offs, qt, d, sens = offs.copy(), qt.copy(), d.copy(), sens.copy()
                item = {"first": ch.first_pair, "n_pairs": n, "offsets": offs, "qt": qt, "dist": d, "sensitive": sens,
                        "d_qt": ch.d_qt, "d_dist": ch.d_dist}
                if verified and self._selection_ran():
                    item["model_selection"] = self.model_selection(n)
                if verified and self._two_view_ran():
                    item["two_view_geometry"] = self.two_view_geometry(n)
                    if self._two_view_refinement_ran():
                        item["two_view_refinements"] = self.two_view_refinements(n)
                yield item
        finally:
            # a consumer that breaks out of the loop (GeneratorExit) or whose body raises must not leave the series open: the store
            # would stay locked for uploads until the next matching call
            if not done and getattr(self, "_h", None) and self._series == mine:
                self._L.msfm_match_pairs_end(self._h)

    def memory_info(self):
        """Bytes the context holds (store, inbox, scratch, result lists, page-locked host) + the device's free / total memory."""
        m = Memory()
        self._chk(self._L.msfm_memory_info(self._h, C.byref(m)))
        return _dict(m)

    def read_device(self, dev_ptr, shape, dtype):
        """A device buffer (raw pointer) as a new NumPy array, copied through the library's own runtime."""
        out = np.empty(shape, dtype)
        self._chk(self._L.msfm_read_device(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dev_ptr), out.nbytes))
        return out

    def fetch_matches_device(self, qt_ptr, dist_ptr=None):
        """Copy the last call's lists into caller-owned DEVICE memory on this context's GPU (raw pointers, e.g.
        torch.Tensor.data_ptr() of an int32 [M, 2] / float32 [M] tensor; None skips one)."""
        self._chk(self._L.msfm_fetch_matches_device(self._h, C.c_void_p(qt_ptr or 0), C.c_void_p(dist_ptr or 0)))

    def order_certificate(self, n_pairs):
        """Per pair of the last match_pairs call: rows / columns whose decisions are within the fp32 reassociation bound
        of flipping under another accumulation order (0 everywhere: the index lists are order-invariant)."""
        out = np.zeros(max(int(n_pairs), 1), np.int32)
        self._chk(self._L.msfm_fetch_order_certificate(self._h, _ip(out)))
        return out[:int(n_pairs)]

    def upload_keypoints(self, image_id, kpts):
        """kpts: n x k float32 (k >= 2), x and y in the first two columns."""
        kpts = np.ascontiguousarray(kpts, dtype=np.float32)
        if kpts.ndim != 2 or kpts.shape[1] < 2:
            raise ValueError("keypoints must be n x (>=2)")
        self._chk(self._L.msfm_upload_keypoints(self._h, int(image_id), _fp(kpts), kpts.shape[0], kpts.shape[1]))

    def match_pairs_verified(self, pairs, ratio=0.8, cross_check=True, max_distance=0.7, threshold=3.0,
                             confidence=0.99, max_iters=1000, seed=0x5eed5eed, fetch=True):
        """match_pairs + FeatureUtils::FilterMatches (F-matrix RANSAC) on the device."""
        return self._match(pairs, MatchParams(ratio, int(bool(cross_check)), max_distance),
                           VerifyParams(threshold, confidence, int(max_iters), int(seed)), fetch)

    def set_verification_model(self, model, camera=None):
        """Model of the geometric verification of match_pairs_verified and the verified streaming form: VERIFY_FUNDAMENTAL (0,
        the default: FeatureUtils::FilterMatches), VERIFY_ESSENTIAL (1: 5-point essential-matrix RANSAC with `camera`, a dict
        or sequence fx, fy, cx, cy[, k1, k2, p1, p2] -- missing distortion coefficients are 0) or VERIFY_HOMOGRAPHY (2: 4-point
        homography RANSAC on pixel coordinates, for planar scenes and rotation-only views; it takes no camera, and a given one is
        passed on and refused with E_INVALID)."""
        cam = camera_struct(camera) if camera is not None else None
        self._chk(self._L.msfm_set_verification_model(self._h, int(model), C.byref(cam) if cam is not None else None))

    def verification_stats(self):
        """(hypotheses solved, rounds run) of the last verified call / series under VERIFY_ESSENTIAL or VERIFY_HOMOGRAPHY."""
        solved, rounds = C.c_int64(), C.c_int()
        self._chk(self._L.msfm_get_verification_stats(self._h, C.byref(solved), C.byref(rounds)))
        return int(solved.value), int(rounds.value)

    def set_model_selection(self, enable=True, h_ratio=0.7):
        """The two-view model selection of the verified calls (include/msfm_match.h): under VERIFY_FUNDAMENTAL or VERIFY_ESSENTIAL every
        pair also runs the homography and keeps the homography's list iff nE > 0 and nH >= h_ratio * nE, else the epipolar one.
        No effect under VERIFY_HOMOGRAPHY.  A bad h_ratio (not finite, <= 0) is E_INVALID; E_STATE while a series is open."""
        self._chk(self._L.msfm_set_model_selection(self._h, int(bool(enable)), float(h_ratio)))

    def model_selection(self, n_pairs):
        """Per pair of the last match_pairs_verified call (or of the last verified stream chunk): (model kept, nE, nH), three int32
        arrays.  E_STATE if that call ran without the selection."""
        n = int(n_pairs)
        out = [np.zeros(max(n, 1), np.int32) for _ in range(3)]
        self._chk(self._L.msfm_fetch_model_selection(self._h, *[_ip(a) for a in out]))
        return tuple(a[:n] for a in out)

    def _selection_ran(self):
        return self._L.msfm_fetch_model_selection(self._h, None, None, None) == OK

    def set_two_view_geometry(self, enable=True, min_num_inliers=100, tri_max_error=2.0, tri_min_angle=4.0):
        """The two-view geometry of the verified calls under VERIFY_ESSENTIAL (include/msfm_match.h): every pair also gets a record
        with the relative pose of its winning E, the triangulation statistics of its kept matches and the reference's test for an
        initial pair (defaults: the reference's).  The lists do not change.  E_INVALID for a negative / non-finite parameter or under
        another model; E_STATE while a series is open."""
        prm = TwoViewParams(int(min_num_inliers), 0, float(tri_max_error), float(tri_min_angle))
        self._chk(self._L.msfm_set_two_view_geometry(self._h, int(bool(enable)), C.byref(prm)))

    def two_view_geometry(self, n_pairs):
        """Per pair of the last match_pairs_verified call (or of the last verified stream chunk): a structured array of dtype
        TWO_VIEW_RECORD.  E_STATE if that call ran without the two-view geometry."""
        n = int(n_pairs)
        out = np.zeros(max(n, 1), TWO_VIEW_RECORD)
        self._chk(self._L.msfm_fetch_two_view_geometry(self._h, out.ctypes.data))
        return out[:n]

    def _two_view_ran(self):
        return self._L.msfm_fetch_two_view_geometry(self._h, None) == OK

    def set_two_view_refinement(self, enable=True, max_iters=10, step_tol=1e-6, min_matches=15):
        """The two-view pose refinement behind the two-view geometry (include/msfm_match.h): the pose of every valid record with at
        least min_matches kept matches is polished by LM on the Sampson error over all its kept matches, and the refined record
        replaces the record iff a step was accepted and neither count of the record drops.  The lists do not change.  E_INVALID for
        max_iters < 1, min_matches < 5, a negative / non-finite step_tol or while the two-view geometry is off; E_STATE while a
        series is open."""
        prm = TwoViewRefineParams(int(max_iters), int(min_matches), float(step_tol))
        self._chk(self._L.msfm_set_two_view_refinement(self._h, int(bool(enable)), C.byref(prm)))

    def two_view_refinements(self, n_pairs):
        """Per pair of the last match_pairs_verified call (or of the last verified stream chunk): a structured array of dtype
        TWO_VIEW_REFINEMENT (two_view_refined gives the mask of the replaced records).  E_STATE if that call ran without the
        refinement."""
        n = int(n_pairs)
        out = np.zeros(max(n, 1), TWO_VIEW_REFINEMENT)
        self._chk(self._L.msfm_fetch_two_view_refinements(self._h, out.ctypes.data))
        return out[:n]

    def _two_view_refinement_ran(self):
        return self._L.msfm_fetch_two_view_refinements(self._h, None) == OK

    # ---- feature tracks (include/msfm_match.h) ----
    def tracks_begin(self, ids, min_pair_matches=0, add_only=False):
        """Open a track session over the resident images `ids`: from now on every match_pairs / match_pairs_verified call and every
        chunk of match_pairs_stream folds the lists it hands out into one union-find forest on the device.  A pair with fewer than
        min_pair_matches matches contributes nothing (0: every pair; the reference's SceneGraph::Load uses 10).  add_only: the matching
        calls do not fold, only tracks_add / tracks_import_forest do."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        prm = TrackParams(int(min_pair_matches), int(bool(add_only)))
        self._chk(self._L.msfm_tracks_begin(self._h, _ip(ids), len(ids), C.byref(prm)))
        self._track_nodes = int(sum(self.image_rows(int(i)) for i in ids))
        self._track_ids = [int(i) for i in ids]   # (grow()'s default list)

    def tracks_add(self, pairs, offsets, qt):
        """Fold host lists in (CSR as match_pairs returns them: pairs P x 2, offsets P + 1, qt M x 2).  An index outside its image's
        rows and a pair with id1 == id2 are ignored and counted, a pair with an undeclared image is skipped and counted."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        qt = np.ascontiguousarray(np.asarray(qt, dtype=np.int32).reshape(-1, 2))
        if len(offsets) != len(pairs) + 1 or (len(pairs) and int(offsets[-1]) > len(qt)):
            raise ValueError("offsets must have P + 1 entries within qt")
        self._chk(self._L.msfm_tracks_add(self._h, _ip(pairs), len(pairs), offsets.ctypes.data_as(C.POINTER(C.c_int64)), _ip(qt)))

    def tracks_finish(self, min_length=2, max_length=0, keep_inconsistent=False):
        """Close the accumulation and build the tracks under the filter (may be called again with another filter) -> stats dict."""
        f = TrackFilter(int(min_length), int(max_length), int(bool(keep_inconsistent)), 0)
        st = TrackStats()
        self._chk(self._L.msfm_tracks_finish(self._h, C.byref(f), C.byref(st)))
        self._track_stats = _dict(st)
        return dict(self._track_stats)

    def _kept(self):
        """(kept tracks, kept observations) of the last tracks_finish; (0, 0) without one."""
        st = getattr(self, "_track_stats", None) or {}
        return int(st.get("tracks_kept", 0)), int(st.get("observations_kept", 0))

    def tracks(self):
        """-> (offsets[T + 1] int64, image_ids[O] int32, point_idx[O] int32, consistent[T] uint8) of the last tracks_finish: kept tracks
        by ascending smallest (image id, keypoint index), the elements of each in that order."""
        T, O = self._kept()
        offs = np.zeros(T + 1, np.int64)
        img, idx = np.zeros(max(O, 1), np.int32), np.zeros(max(O, 1), np.int32)
        cons = np.zeros(max(T, 1), np.uint8)
        self._chk(self._L.msfm_fetch_tracks(self._h, offs.ctypes.data_as(C.POINTER(C.c_int64)), _ip(img), _ip(idx),
                                            cons.ctypes.data_as(C.POINTER(C.c_uint8))))
        return offs, img[:O], idx[:O], cons[:T]

    def track_ids(self, image_id):
        """Per keypoint of a declared image: the number of its kept track or -1."""
        n = self.image_rows(image_id)
        out = np.full(max(n, 1), -1, np.int32)
        self._chk(self._L.msfm_fetch_track_ids(self._h, int(image_id), _ip(out)))
        return out[:n]

    def tracks_export_forest(self):
        """The session's forest: one int32 per node (the declared images' rows, images by ascending id), each a node of the same
        component."""
        nodes = int(getattr(self, "_track_nodes", 0) or 0)
        out = np.zeros(max(nodes, 1), np.int32)
        self._chk(self._L.msfm_tracks_export_forest(self._h, _ip(out)))
        return out[:nodes]

    def tracks_import_forest(self, parent):
        """Join every node v with parent[v] (a forest exported by a session over the same images, e.g. on another GPU)."""
        parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        nodes = getattr(self, "_track_nodes", None)   # (None: no session was opened through this object -- the library says so)
        if nodes is not None and len(parent) != nodes:
            raise ValueError("the forest must have one entry per node of the session (%d), got %d" % (nodes, len(parent)))
        self._chk(self._L.msfm_tracks_import_forest(self._h, _ip(parent)))

    def tracks_end(self):
        self._track_stats = None
        self._track_nodes = None
        self._chk(self._L.msfm_tracks_end(self._h))

    # ---- track triangulation (include/msfm_match.h) ----
    def triangulate_tracks(self, camera, poses, max_error=2.0, min_angle=1.5, min_views=2, robust=False, max_hypotheses=64):
        """3-D points of the kept tracks of the last tracks_finish under known poses: camera as set_verification_model takes it, poses a
        dict image id -> (R, t) with x_cam = R X + t (None: listed but unposed; declared images that are not listed are unposed too),
        listed by ascending id, or a pair (ids, POSE_RT array) as pose_list() returns it, listed in the given order (pose_list(),
        pose_refinements() and the cost sums of refine_poses follow the list's order; nothing else depends on it).
        Defaults: the reference's Triangulator::Parameters.  -> stats dict.  The points are fetched with points3d().
        robust=True: msfm_triangulate_tracks_robust -- a track whose plain point fails the error test is retried over at most
        max_hypotheses two-view hypotheses and keeps the observations that agree; the stats dict gains msfm_robust_stats' fields and
        point_inliers() returns the inlier byte of every observation."""
        cam = camera_struct(camera) if camera is not None else None
        ids, tab = pose_table(poses)
        st = TriangulationStats()
        self._tri_route = int(max_hypotheses) if robust else 0   # (what extend_points(max_hypotheses=None) follows)
        self._tri_thresholds = (float(max_error), float(min_angle))   # (what filter_points() without thresholds follows)
        if robust:
            rprm = RobustTriangulationParams(float(max_error), float(min_angle), int(min_views), int(max_hypotheses))
            rs = RobustStats()
            self._chk(self._L.msfm_triangulate_tracks_robust(self._h, C.byref(cam) if cam is not None else None, _ip(ids), tab.ctypes.data,
                                                             len(ids), C.byref(rprm), C.byref(st), C.byref(rs)))
            out = _dict(st)
            out.update(_dict(rs))
            return out
        prm = TriangulationParams(float(max_error), float(min_angle), int(min_views), 0)
        self._chk(self._L.msfm_triangulate_tracks(self._h, C.byref(cam) if cam is not None else None, _ip(ids), tab.ctypes.data, len(ids),
                                                  C.byref(prm), C.byref(st)))
        return _dict(st)

    def point_inliers(self):
        """-> uint8, one per kept observation in the tracks' order (aligned with points3d()'s residuals): 1 where the observation
        supports its track's point.  Only after triangulate_tracks(..., robust=True)."""
        O = self._kept()[1]
        out = np.zeros(max(O, 1), np.uint8)
        self._chk(self._L.msfm_fetch_point_inliers(self._h, out.ctypes.data))
        return out[:O]

    def refine_points(self, max_iters=10, step_tol=1e-10):
        """Moves every point of the last triangulate_tracks to the minimum of its reprojection error under that call's poses (per-track
        Levenberg-Marquardt, msfm_refine_points); a refined point replaces its record only where it costs strictly less and clears no
        status bit.  -> stats dict.  points3d() and point_inliers() work after it unchanged; refined(points) is the mask of the
        records it rewrote.  Registrations are invalidated as by triangulate_tracks."""
        prm = RefineParams(float(step_tol), int(max_iters), 0)
        st = RefineStats()
        self._chk(self._L.msfm_refine_points(self._h, C.byref(prm), C.byref(st)))
        return _dict(st)

    def refine_poses(self, max_iters=10, step_tol=1e-6, min_observations=15, fixed=()):
        """Moves every posed image of the last triangulate_tracks to the minimum of its reprojection error under the current points
        (per-image Levenberg-Marquardt, msfm_refine_poses); `fixed`: image ids whose pose is held.  A refined pose replaces the
        session's only where it costs strictly less and loses no inlier; the records of the tracks it touches are evaluated again
        (reposed(points)).  -> stats dict.  poses() returns the current poses, pose_refinements() the per-image records.
        Registrations are invalidated as by refine_points."""
        prm = PoseRefineParams(float(step_tol), int(max_iters), int(min_observations))
        st = PoseRefineStats()
        fx = np.ascontiguousarray(list(fixed), dtype=np.int32).reshape(-1)
        self._chk(self._L.msfm_refine_poses(self._h, C.byref(prm), _ip(fx) if len(fx) else None, len(fx), C.byref(st)))
        return _dict(st)

    def pose_list(self):
        """-> (ids int32, POSE_RT array) of the session's current pose list, in the order of the triangulation call."""
        n = C.c_int(0)
        self._chk(self._L.msfm_fetch_poses(self._h, None, None, C.byref(n)))
        ids, tab = np.zeros(max(n.value, 1), np.int32), np.zeros(max(n.value, 1), POSE_RT)
        self._chk(self._L.msfm_fetch_poses(self._h, _ip(ids), tab.ctypes.data, C.byref(n)))
        return ids[:n.value], tab[:n.value]

    def poses(self):
        """-> {image id: (R, t)} of the session's valid poses: what triangulate_tracks was given, with every pose that a refine_poses
        call has replaced since.  The form triangulate_tracks takes."""
        ids, tab = self.pose_list()
        return {int(i): (p["R"].reshape(3, 3).copy(), p["t"].copy()) for i, p in zip(ids, tab) if p["valid"]}

    def pose_refinements(self):
        """-> POSE_REFINEMENT array, one record per listed image, of the last refine_poses."""
        n = C.c_int(0)
        self._chk(self._L.msfm_fetch_poses(self._h, None, None, C.byref(n)))
        rec = np.zeros(max(n.value, 1), POSE_REFINEMENT)
        self._chk(self._L.msfm_fetch_pose_refinements(self._h, rec.ctypes.data))
        return rec[:n.value]

    def refine_camera(self, mask=("fx_fy",), max_iters=10, step_tol=1e-6, min_observations=100):
        """Moves the session's one camera to the minimum of the map's reprojection error under the current poses and points (one
        6 x 6 Levenberg-Marquardt, msfm_refine_camera).  mask: the unknowns -- names out of "fx_fy" (the default), "f" (one common
        scale; not with "fx_fy"), "cx_cy", "k1_k2", or the MSFM_CAM_* bits.  The refined camera replaces the session's only where it
        costs strictly less and loses no inlier; every point's record is then evaluated again (recalibrated(points)).  -> stats dict,
        camera_before / camera_after as dicts.  camera() returns the current camera: pass it to register_images.  Registrations and
        pose refinements are invalidated as by refine_points."""
        prm = CameraRefineParams(float(step_tol), camera_mask(mask), int(max_iters), int(min_observations), 0)
        st = CameraRefineStats()
        self._chk(self._L.msfm_refine_camera(self._h, C.byref(prm), C.byref(st)))
        out = _dict(st)
        out["camera_before"], out["camera_after"] = camera_dict(st.camera_before), camera_dict(st.camera_after)
        return out

    def camera(self):
        """-> the session's current camera as a dict (the form every call takes): what triangulate_tracks was given, or what the last
        refine_camera that stood left."""
        cam = Camera()
        self._chk(self._L.msfm_fetch_camera(self._h, C.byref(cam)))
        return camera_dict(cam)

    def alternate(self, rounds, fixed=(), point_params=None, pose_params=None, camera_params=None):
        """`rounds` times refine_points(**point_params) then refine_poses(fixed=fixed, **pose_params); stops early after a round that
        refined neither a point nor a pose.  -> [(point stats, pose stats)] per round run.
        camera_params: a dict (may be empty) runs refine_camera(**camera_params) behind the pose call of every round; the list then
        holds (point stats, pose stats, camera stats) and the early stop needs a camera that did not stand as well."""
        out = []
        for _ in range(int(rounds)):
            a = self.refine_points(**(point_params or {}))
            b = self.refine_poses(fixed=fixed, **(pose_params or {}))
            stats = (a, b) if camera_params is None else (a, b, self.refine_camera(**camera_params))
            out.append(stats)
            if all(s["refined"] == 0 for s in stats):
                break
        return out

    def extend_points(self, poses, max_hypotheses=None):
        """Brings newly posed images into the map without a full triangulation (msfm_extend_points): `poses` -- a dict or an (ids,
        POSE_RT) pair as triangulate_tracks takes them -- lists ONLY images that have no valid pose in the session yet.  Standing points
        (POINT & ERROR_OK & ANGLE_OK) are continued into the new images without moving; every other consistent track that sees a new
        image is triangulated afresh under the enlarged pose list; tracks that see none stay bit for bit.  max_hypotheses: 0 = the
        plain route for the created tracks, 1 .. 1024 = the robust one, None = the route of this context's last triangulate_tracks.
        -> stats dict.  extended(points) is the mask of the records it continued or created; pose_list() returns the enlarged list and
        point_inliers() works after it whatever the triangulation was.  Registrations and pose refinements are invalidated."""
        ids, tab = pose_table(poses)
        if max_hypotheses is None:
            max_hypotheses = getattr(self, "_tri_route", 0)
        prm = ExtendParams(int(max_hypotheses), 0)
        st = ExtendStats()
        self._chk(self._L.msfm_extend_points(self._h, _ip(ids) if len(ids) else None, tab.ctypes.data if len(ids) else None, len(ids),
                                             C.byref(prm), C.byref(st)))
        return _dict(st)

    # ---- map visibility (include/msfm_match.h) ----
    def visibility(self, query=(), basis="map", route="auto"):
        """Covisibility counts of the session on the device (msfm_map_visibility), read-only: basis "tracks" counts the kept consistent
        tracks of the last tracks_finish (no points needed), "map" the standing points and, in a posed image, only their fitting
        observations.  query: the image ids whose rows of the matrix are wanted.  route: "auto", "global" or "lds" (the same counts).
        -> (records: VISIBILITY array, one per declared image by ascending id; matrix: uint32 [len(query), n], matrix[r, j] = the
        standing tracks query[r] shares with the image of records[j], its own count at its own column; stats dict).  next_images,
        local_window, initial_first_images and initial_second_images order them as the reference's MapBuilder does."""
        q = np.ascontiguousarray([int(i) for i in query], dtype=np.int32).reshape(-1)
        n = len(getattr(self, "_track_ids", None) or ())
        prm = VisibilityParams(_VIS_BASES[basis], _VIS_ROUTES[route])
        rec = np.zeros(max(n, 1), VISIBILITY)
        mat = np.zeros((len(q), n), np.uint32)
        st = VisibilityStats()
        self._chk(self._L.msfm_map_visibility(self._h, C.byref(prm), _ip(q) if len(q) else None, len(q), rec.ctypes.data,
                                              mat.ctypes.data if mat.size else None, C.byref(st)))
        return rec[:n], mat, _dict(st)

    # ---- map alignment (include/msfm_match.h) ----
    def estimate_alignment(self, positions, max_error=None, confidence=0.9999, max_hypotheses=1024, min_inliers=3):
        """The similarity world' = s Q X + d that takes the session's camera centres to known positions (msfm_estimate_alignment),
        read-only.  positions: {image id: (x, y, z)}; an image without a valid pose in the session is reported as not used.
        max_error, in the positions' units: a prior is an inlier iff its error is at most that, and the estimate is robust (three-prior
        hypotheses, at most max_hypotheses of them under `confidence`, then refits over the inliers).  max_error=None: one least-squares
        fit of all usable priors.  Subtract a local origin from large coordinates (UTM) first.
        -> (dict: status (ALN_* bits), n_listed, n_used, n_inliers, hypotheses, refits, s, Q, d, rms, estimate_ms;
            ALIGNMENT_RESIDUAL array, one per prior by ascending image id: flags (ALN_USED | ALN_INLIER), error).  A failed estimate
        has ALN_SUCCEEDED clear and s = 0."""
        ids, pos = prior_table(positions)
        robust = max_error is not None
        prm = AlignmentParams(float(max_error) if robust else 0.0, float(confidence), int(max_hypotheses) if robust else 0, int(min_inliers))
        out = Alignment()
        rec = np.zeros(max(len(ids), 1), ALIGNMENT_RESIDUAL)
        self._chk(self._L.msfm_estimate_alignment(self._h, _ip(ids) if len(ids) else None,
                                                  pos.ctypes.data_as(C.POINTER(C.c_double)) if len(ids) else None, len(ids), C.byref(prm),
                                                  C.byref(out), rec.ctypes.data))
        return alignment_dict(out), rec[:len(ids)]

    def transform_map(self, s, Q, d):
        """Moves the whole map by the similarity world' = s Q X + d (msfm_transform_map): every valid pose becomes R Q^T, s t - R' d,
        every point s Q X + d, and every point's record is evaluated again under the new poses (aligned(points)); projections do not
        change.  Any valid similarity is taken: estimate_alignment's or the caller's own.  -> stats dict.  pose_list(), points3d(),
        point_inliers() and camera() work after it; registrations and pose refinements are invalidated."""
        g = similarity_struct(s, Q, d)
        st = TransformStats()
        self._chk(self._L.msfm_transform_map(self._h, C.byref(g), C.byref(st)))
        return _dict(st)

    def align(self, positions, **estimate_kwargs):
        """estimate_alignment(positions, **estimate_kwargs), then transform_map(its similarity) iff it succeeded.
        -> (alignment dict, per-prior records, transform stats or None)."""
        a, rec = self.estimate_alignment(positions, **estimate_kwargs)
        if not a["status"] & ALN_SUCCEEDED:
            return a, rec, None
        return a, rec, self.transform_map(a["s"], a["Q"], a["d"])

    def initialize(self, camera, two_view, max_trials=100, min_points=100, **triangulate_kwargs):
        """The reference's TryInitialize order over the finished tracks: first images by their number of track elements
        (initial_first_images), per first image one visibility([id], basis="tracks") and its second images by the tracks they share
        with it (initial_second_images).  two_view: {(id1, id2): TWO_VIEW_RECORD}; a pair is a trial iff its record exists (under
        either key order), is valid and has is_initial_candidate.  A trial calls triangulate_tracks(camera, ...) with the record's
        first image at (I, 0) and its second at the record's (R, t) and succeeds when the call's `succeeded` reaches min_points (100:
        the two-view parameters' min_num_inliers default); at most max_trials trials (100: the reference's max_num_init_trials).
        -> (the record's (id1, id2) or None, trials run, the last trial's stats or None)."""
        records = self.visibility(basis="tracks")[0]
        trials, stats, tried = 0, None, set()
        for a in initial_first_images(records):
            if trials >= int(max_trials):
                break
            rec_a, mat, _ = self.visibility([a], basis="tracks")
            for b in initial_second_images(mat[0], rec_a, a):
                if trials >= int(max_trials):
                    break
                key = (a, b) if (a, b) in two_view else (b, a)
                if key not in two_view or key in tried:
                    continue
                tv = two_view[key]
                if not (int(tv["valid"]) and int(tv["is_initial_candidate"])):
                    continue
                tried.add(key)
                trials += 1
                poses = {key[0]: (np.eye(3), np.zeros(3)), key[1]: (np.asarray(tv["R"], np.float64).reshape(3, 3), np.asarray(tv["t"], np.float64))}
                stats = self.triangulate_tracks(camera, poses, **triangulate_kwargs)
                if stats["succeeded"] >= int(min_points):
                    return key, trials, stats
        return None, trials, stats

    def grow(self, camera, image_ids=None, register_params=None, rounds=1, fixed=(), point_params=None, pose_params=None, max_images=None,
             window=None, camera_params=None):
        """One increment of the reconstruction: register_images(camera, image_ids, **register_params) -- image_ids None: every declared
        image without a valid pose in the session -- then extend_points(the registered poses), then alternate(rounds, fixed=...).
        -> (register stats, extend stats or None, alternate's list, the ids that registered).  When no image registers nothing but the
        registrations has changed and the call returns early.
        max_images=k (image_ids None): the candidates are next_images(visibility()[0]) -- the unposed images that see enough of the
        map, best-seen first -- tried in batches of k until a batch registers something or the list ends.  window=w: behind
        extend_points one visibility(query=the new ids); alternate holds every posed image fixed that is neither new nor in a new
        image's local_window(..., size=w).  max_images=1, window=5 is the reference's loop; both None: every call as before.
        camera_params: a dict (may be empty) is passed on to alternate, and register_images then runs under self.camera() -- the
        session's current camera, which an earlier increment may have refined -- in place of `camera`."""
        if image_ids is None and max_images is not None:
            cand = next_images(self.visibility()[0])
            batches = [cand[k:k + int(max_images)] for k in range(0, len(cand), max(int(max_images), 1))]
        else:
            if image_ids is None:
                posed = set(self.poses())
                image_ids = [int(i) for i in sorted(getattr(self, "_track_ids", ())) if int(i) not in posed]
            batches = [[int(i) for i in image_ids]]
        reg, new = None, {}
        for batch in batches:
            if not batch:
                continue
            reg = self.register_images(camera if camera_params is None else self.camera(), batch, **(register_params or {}))
            new = registered_poses(self.registrations()[0])
            if new:
                break
        if not new:
            return reg, None, [], []
        ext = self.extend_points(new)
        if window is not None:
            records, mat, _ = self.visibility(query=sorted(new))
            inside = set(new)
            for row, i in zip(mat, sorted(new)):
                inside.update(local_window(row, records, i, size=window))
            outside = [int(r["image_id"]) for r in records if (r["flags"] & VIS_POSED) and int(r["image_id"]) not in inside]
            fixed = sorted(set(int(i) for i in fixed) | set(outside))
        alt = self.alternate(rounds, fixed=fixed, point_params=point_params, pose_params=pose_params, camera_params=camera_params)
        return reg, ext, alt, sorted(new)

    def filter_points(self, max_error=None, min_angle=None, image_ids=None):
        """Takes observations that no longer fit their point out of its fitting set and removes the points left with fewer than two
        observations or without a pair of views min_angle apart (msfm_filter_points); no point and no pose moves.  max_error in pixels,
        min_angle in degrees; if either is None both are those of this context's last triangulate_tracks.  image_ids: only the tracks
        with a fitting observation in a listed image (None or empty: every track).  -> stats dict.  filtered(points) is the mask of the
        records it trimmed or removed; point_inliers() works after it whatever the triangulation was.  Registrations and pose
        refinements are invalidated."""
        prm = None
        if max_error is not None and min_angle is not None:
            prm = FilterParams(float(max_error), float(min_angle))
        elif getattr(self, "_tri_thresholds", None) is not None:
            prm = FilterParams(*self._tri_thresholds)
        ids = np.ascontiguousarray(list(image_ids) if image_ids is not None else [], dtype=np.int32).reshape(-1)
        st = FilterStats()
        self._chk(self._L.msfm_filter_points(self._h, C.byref(prm) if prm is not None else None, _ip(ids) if len(ids) else None, len(ids),
                                             C.byref(st)))
        return _dict(st)

    def complete_points(self, max_error=None, image_ids=None):
        """Tests the observations of the standing points whose inlier byte is 0 again and re-admits those that fit under the current
        poses (msfm_complete_points); no point and no pose moves.  max_error in pixels, at most that of this context's last
        triangulate_tracks; None = that value (NULL parameters).  image_ids: only the candidates in a listed image (None or empty:
        every image).  -> stats dict.  completed(points) is the mask of the records it admitted an observation into; point_inliers()
        works after it whatever the triangulation was.  Registrations and pose refinements are invalidated."""
        prm = CompleteParams(float(max_error)) if max_error is not None else None
        ids = np.ascontiguousarray(list(image_ids) if image_ids is not None else [], dtype=np.int32).reshape(-1)
        st = CompleteStats()
        self._chk(self._L.msfm_complete_points(self._h, C.byref(prm) if prm is not None else None, _ip(ids) if len(ids) else None, len(ids),
                                               C.byref(st)))
        return _dict(st)

    def reconstruct(self, camera, rounds=1, filter_params=None, max_increments=None, complete_params=None, **grow_kwargs):
        """The reference's DoBuild loop with its filter: grow(camera, rounds=rounds, **grow_kwargs) followed by
        filter_points(**filter_params), repeated until no image registers or max_increments increments have run.  complete_params: a
        dict (may be empty) runs complete_points(**complete_params) behind the filter of every increment; None: no completion.
        grow's max_images=1, window=5 make it the reference's loop in order as well: one image an increment, best-seen first, the new
        image and its five most covisible neighbours adjusted.  grow's camera_params={...} adds refine_camera to every round of the
        alternation and registers every increment under the session's current camera.
        -> one dict per increment: register, extend, alternate (grow's results), filter (filter_points' stats), registered (the ids),
        and with complete_params "complete" (complete_points' stats)."""
        out = []
        while max_increments is None or len(out) < int(max_increments):
            reg, ext, alt, new = self.grow(camera, rounds=rounds, **grow_kwargs)
            if not new:
                break
            flt = self.filter_points(**(filter_params or {}))
            out.append({"register": reg, "extend": ext, "alternate": alt, "filter": flt, "registered": new})
            if complete_params is not None:
                out[-1]["complete"] = self.complete_points(**complete_params)
        return out

    def points3d(self):
        """-> (points: POINT3D array, one per kept track; residuals: float64, one per kept observation in the tracks' order, -1.0 where
        no error was computed) of the last triangulate_tracks.  succeeded(points) is the reference's verdict."""
        T, O = self._kept()
        pts = np.zeros(max(T, 1), POINT3D)
        res = np.zeros(max(O, 1), np.float64)
        self._chk(self._L.msfm_fetch_points3d(self._h, pts.ctypes.data, res.ctypes.data_as(C.POINTER(C.c_double))))
        return pts[:T], res[:O]

    # ---- image registration (include/msfm_match.h) ----
    def register_images(self, camera, image_ids, max_error=4.0, confidence=0.9999, max_iters=1024, min_inliers=15, refine_iters=10):
        """Absolute poses of the listed images from their correspondences with the points of the last triangulate_tracks: P3P RANSAC
        and a Gauss-Newton refinement per image, all images in one call.  Defaults: the reference's Registrant parameters.  -> stats
        dict.  The records are fetched with registrations()."""
        cam = camera_struct(camera) if camera is not None else None
        ids = np.ascontiguousarray(image_ids, dtype=np.int32).reshape(-1)
        prm = RegisterParams(float(max_error), float(confidence), int(max_iters), int(min_inliers), int(refine_iters), 0)
        st = RegisterStats()
        self._reg_shape = None
        self._chk(self._L.msfm_register_images(self._h, C.byref(cam) if cam is not None else None, _ip(ids), len(ids), C.byref(prm),
                                               C.byref(st)))
        self._reg_shape = (len(ids), int(st.correspondences))
        return _dict(st)

    def registrations(self):
        """-> (records: REGISTRATION array in the order of the list, offsets[n + 1] int64, track_ids int32, inlier uint8, residuals
        float64 per correspondence) of the last register_images.  registered(records) is the reference's verdict;
        registered_poses(records, poses) the pose dict for the next triangulate_tracks."""
        n, m = getattr(self, "_reg_shape", None) or (0, 0)
        rec = np.zeros(max(n, 1), REGISTRATION)
        offs = np.zeros(n + 1, np.int64)
        tid, inl, res = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.uint8), np.zeros(max(m, 1), np.float64)
        self._chk(self._L.msfm_fetch_registrations(self._h, rec.ctypes.data, offs.ctypes.data, tid.ctypes.data, inl.ctypes.data,
                                                   res.ctypes.data))
        return rec[:n], offs, tid[:m], inl[:m], res[:m]

    def knn2_pair(self, id1, id2):
        n1, n2 = self.image_rows(id1), self.image_rows(id2)
        f_i = np.empty(max(n1, 1), np.int32)
        f_d0 = np.empty(max(n1, 1), np.float32)
        f_d1 = np.empty(max(n1, 1), np.float32)
        r_i = np.empty(max(n2, 1), np.int32)
        r_d0 = np.empty(max(n2, 1), np.float32)
        r_d1 = np.empty(max(n2, 1), np.float32)
        self._chk(self._L.msfm_knn2_pair(self._h, int(id1), int(id2), _ip(f_i), _fp(f_d0), _fp(f_d1),
                                         _ip(r_i), _fp(r_d0), _fp(r_d1)))
        return (f_i[:n1], f_d0[:n1], f_d1[:n1]), (r_i[:n2], r_d0[:n2], r_d1[:n2])


def device_count():
    """gfx950 devices msfm_create can open (0 without a GPU)."""
    return int(load().msfm_device_count())


def topscale_select(kpts, k):
    L = load()
    kpts = np.ascontiguousarray(kpts, dtype=np.float32).reshape(-1, 4)
    n = kpts.shape[0]
    out = np.empty(max(n, 1), np.int32)
    cnt = C.c_int()
    rc = L.msfm_topscale_select(_fp(kpts), n, int(k), _ip(out), C.byref(cnt))
    if rc != OK:
        raise MsfmError(rc, "msfm_topscale_select")
    return out[:cnt.value].copy()


def pair_id(id1, id2):
    L = load()
    out = C.c_int32()
    rc = L.msfm_pair_id(int(id1), int(id2), C.byref(out))
    if rc != OK:
        raise MsfmError(rc, "msfm_pair_id: ids must be in [0, %d)" % MAX_IMAGES)
    return out.value


def pair_from_id(pid):
    L = load()
    a, b = C.c_int(), C.c_int()
    rc = L.msfm_pair_from_id(int(pid), C.byref(a), C.byref(b))
    if rc != OK:
        raise MsfmError(rc, "msfm_pair_from_id")
    return a.value, b.value


def swap_image_pair(id1, id2):
    return bool(load().msfm_swap_image_pair(int(id1), int(id2)))
