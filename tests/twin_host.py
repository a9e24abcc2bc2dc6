"""The one boundary between the twin drivers (tests/*_twin.py) and libmsfm_host.so: the loader with every twin export's declaration,
the ctypes mirror of host_map (monocularsfm_amd/host/HostTwinMap.h), the packer that fills it from a session's arrays, and the runner
that cuts a per-track twin into slices on a thread pool.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
WORKERS = 16   # a fixed pool: the machine's CPU count says nothing about the CPUs this process may use

# msfm_pose_rt (104 bytes) and msfm_point3d (48 bytes) of include/msfm_match.h: the binding's dtypes and its pose-list builder, not copies
from monocularsfm_amd._lib import POINT3D, POSE_RT, pose_table  # noqa: E402

assert POSE_RT.itemsize == 104 and POINT3D.itemsize == 48
FP, DP, UP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_int)
_vp, _i, _ll, _d, _u64 = C.c_void_p, C.c_int, C.c_longlong, C.c_double, C.c_ulonglong


class HostMap(C.Structure):
    """host_map, field by field (tests/test_twin_host_abi.py holds the two against each other)"""
    _fields_ = [("offsets", _vp), ("image_ids", _vp), ("point_idx", _vp), ("consistent", _vp), ("n_tracks", C.c_int64),
                ("ids", _vp), ("kxy", _vp), ("pose_ids", _vp), ("poses", _vp), ("n_images", C.c_int32), ("n_poses", C.c_int32),
                ("cam", C.c_double * 8), ("max_error", C.c_double), ("min_angle", C.c_double), ("min_views", C.c_int32),
                ("have_mask", C.c_int32), ("first", C.c_int64), ("count", C.c_int64), ("points", _vp), ("residuals", _vp), ("mask", _vp)]


_MP = C.POINTER(HostMap)
# name -> (restype, argtypes) of every export the drivers call: the nine reconstruction twins over host_map (twin_*; the library also
# has them as host_* with raw argument lists -- no driver calls those, tests/test_twin_host_abi.py holds them against the twins), then the pieces and the
# twins of the other stages (registration, two-view geometry, verification)
EXPORTS = {
    "twin_triangulate_tracks": (_i, [_MP]),
    "twin_triangulate_tracks_robust": (_i, [_MP, _i, _vp, _vp]),
    "twin_refine_points": (_i, [_MP, _d, _i, _vp, _vp, _vp]),
    "twin_refine_poses": (_i, [_MP, _d, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "twin_refine_camera": (_i, [_MP, _d, _i, _i, _i, _vp, _vp, _vp]),
    "twin_extend_points": (_i, [_MP, _vp, _i, _i, _vp, _vp]),
    "twin_filter_points": (_i, [_MP, _vp, _i, _d, _d, _vp, _vp]),
    "twin_complete_points": (_i, [_MP, _vp, _i, _d, _vp, _vp]),
    "twin_map_visibility": (_i, [_MP, _vp, _i, _i, _vp, _vp, _vp]),
    "host_tri_centre": (None, [DP, DP, DP]),
    "host_tri_parallax": (_d, [DP, DP, DP]),
    "host_tri_sample2": (None, [_ll, _i, _i, _vp]),
    "host_rc_reduce": (_d, [DP, _ll]),
    "host_vis_route": (None, [_i, _ll, _ll, _ll, _ll, _vp]),
    "host_register_counts": (_i, [_vp, _vp, _ll, _vp, _vp, _i, _vp]),
    "host_register_images": (_i, [_vp, _vp, _vp, _ll, _vp, _vp, _i, _vp, DP, _d, _d, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "host_register_sample3": (None, [_i, _i, _i, _vp]),
    "host_p3p": (_i, [DP, DP, DP, DP]),
    "host_register_refine": (_i, [DP, DP, DP, DP, DP, _i, _i, DP, DP]),
    "host_pose_decompose": (_i, [DP, DP]),
    "host_pose_triangulate": (_i, [DP, _d, _d, _d, _d, DP]),
    "host_pose_evaluate": (None, [DP, _d, _d, _d, _d, _d, DP]),
    "host_pose_acos": (None, [DP, _i, DP]),
    "host_initial_candidate": (_i, [_i, _d, _d, _d, _i, _d, _d]),
    "host_pose_record": (_i, [DP, DP, DP, DP, DP, _i, _d, _i, _d, _d, _vp]),
    "host_two_view_geometry": (_i, [FP, FP, _i, DP, _i, _d, _d, _d, _d, _i, _u64, UP, _vp]),
    "host_emat_undistort": (None, [DP, DP, _i, DP]),
    "host_essential_ransac": (_i, [FP, FP, _i, DP, _d, _d, _i, _u64, UP]),
    "host_homography_ransac": (_i, [FP, FP, _i, _d, _d, _i, _u64, UP]),
    "host_two_view_select": (_i, [FP, FP, _i, _i, DP, _d, _d, _d, _i, _u64, UP, IP]),
    "host_staged_schedule": (_i, [_i, FP, FP, _i, DP, _d, _d, _i, _u64, IP, C.POINTER(_ll)]),
}
_LIB = None


def load():
    """libmsfm_host.so, made and opened once per process, every export of EXPORTS declared."""
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
        lib = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
        for name, (restype, argtypes) in EXPORTS.items():
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, argtypes
        _LIB = lib
    return _LIB


def as_pose_list(poses):
    """a dict as triangulate_tracks takes it, or (ids, POSE_RT array) as Context.pose_list() returns it -> (ids, a copy of the table)"""
    if isinstance(poses, dict):
        return pose_table(poses)
    ids, tab = poses
    return np.ascontiguousarray(ids, np.int32), np.array(tab, POSE_RT)


def poses_dict(ids, tab):
    return {int(i): ((p["R"].reshape(3, 3).copy(), p["t"].copy()) if p["valid"] else None) for i, p in zip(ids, tab)}


def camera8(cam):
    if isinstance(cam, dict):
        cam = tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"))
    return tuple(float(v) for v in cam) + (0.0,) * (8 - len(cam))


def pack(tracks, ids, kps, poses, cam, thresholds, points=None, residuals=None, mask=None, exact=False):
    """tracks = (offsets, image_ids, point_idx[, consistent]) of a finished session over the declared images `ids`; kps: dict or
    sequence (by position in ids) of n x (>= 2) keypoint arrays (None for an image without, or for all of them); poses: dict id ->
    (R, t) / None, an (ids, POSE_RT) pair, or None for an empty list; cam: up to 8 numbers or the binding's dict; thresholds =
    (max_error, min_angle[, min_views]) of the triangulation.  points, residuals, mask: the state, never changed: the twin works on
    copies under one of two policies.  Padded (exact=False): max(T, 1) records and max(O, 1) residuals (zeros where none are given),
    the mask with one byte appended, NULL without one.  exact=True, the map-edit twins': all three sized exactly, so that an index past
    a track's own slots leaves the arrays; without a mask zero bytes and have_mask 0.  Either way the pose list gets a sentinel entry.
    -> (HostMap over all T tracks, the arrays it points into: T, O, points, residuals, mask, pose_ids, poses -- they must outlive it)"""
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    idx = np.ascontiguousarray(tracks[2], np.int32)
    cons = np.ascontiguousarray(tracks[3], np.uint8) if len(tracks) > 3 else None
    ids = np.ascontiguousarray(ids, np.int32)
    T, O = len(offsets) - 1, len(img)
    xy = []   # (the float32 (x, y) arrays must outlive the calls)
    ptrs = (C.c_void_p * max(len(ids), 1))()
    for k, i in enumerate(ids):
        a = None if kps is None else kps[int(i)] if isinstance(kps, dict) else kps[k]
        if a is None:
            continue
        a = np.ascontiguousarray(np.asarray(a, np.float32)[:, :2])
        xy.append(a)
        ptrs[k] = a.ctypes.data
    pid, tab = pose_table({} if poses is None else poses)
    n_poses = len(pid)
    pid = np.concatenate([pid, np.zeros(1, np.int32)])
    tab = np.concatenate([tab, np.zeros(1, POSE_RT)])
    if exact:
        pts = np.array(points[:T], copy=True)
        res = np.array(residuals[:O], np.float64, copy=True)
        m = np.zeros(O, np.uint8) if mask is None else np.array(mask[:O], np.uint8, copy=True)
    else:
        pts = np.zeros(max(T, 1), POINT3D if points is None else points.dtype)
        res = np.zeros(max(O, 1), np.float64)
        if points is not None:
            pts[:T] = points[:T]
        if residuals is not None:
            res[:O] = residuals[:O]
        m = None if mask is None else np.ascontiguousarray(np.concatenate([mask, np.zeros(1, np.uint8)]), np.uint8)
    held = SimpleNamespace(T=T, O=O, points=pts, residuals=res, mask=m, pose_ids=pid[:n_poses], poses=tab[:n_poses],
                           refs=(offsets, img, idx, cons, ids, xy, ptrs, pid, tab))
    block = HostMap(offsets=offsets.ctypes.data, image_ids=img.ctypes.data, point_idx=idx.ctypes.data,
                    consistent=None if cons is None else cons.ctypes.data, n_tracks=T, ids=ids.ctypes.data,
                    kxy=C.cast(ptrs, C.c_void_p), pose_ids=pid.ctypes.data, poses=tab.ctypes.data, n_images=len(ids), n_poses=n_poses,
                    cam=(C.c_double * 8)(*camera8(cam)), max_error=float(thresholds[0]), min_angle=float(thresholds[1]),
                    min_views=int(thresholds[2]) if len(thresholds) > 2 else 0, have_mask=0 if mask is None else 1, first=0, count=T,
                    points=pts.ctypes.data, residuals=res.ctypes.data, mask=None if m is None else m.ctypes.data)
    return block, held


def sliced(block, first, count):
    """the block for tracks [first, first + count): each slice its own copy, all of them over the same arrays"""
    b = HostMap.from_buffer_copy(block)
    b.first, b.count = first, count
    return b


def run_sliced(T, call, select=None, workers=WORKERS):
    """call(first, count) over [0, T) in four slices per worker on a thread pool, or once per track of `select`; serially for one job
    or workers <= 1.  -> {first: what call returned}"""
    if select is None:
        step = max(1, (T + 4 * workers - 1) // (4 * workers))
        jobs = [(f, min(step, T - f)) for f in range(0, T, step)]
    else:
        jobs = [(int(t), 1) for t in select]
    if len(jobs) <= 1 or workers <= 1:
        got = [call(*j) for j in jobs]
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            got = list(pool.map(lambda j: call(*j), jobs))
    return {j[0]: g for j, g in zip(jobs, got)}


def total(parts, *sums):
    """adds the arrays each slice returned to `sums`, slice by slice in ascending `first`: the order reaches the bits of a float sum"""
    for first in sorted(parts):
        for s, p in zip(sums, parts[first]):
            s += p
    return sums


def edit(fn, own, keys, trace_dtype, packed, select, workers, trace, extra=()):
    """The body the map-edit drivers share (extension, filtering, completion): fn(block, *own, counts, trace) per slice of `packed`,
    what pack(.., exact=True) returned.  -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of `keys`, `extra`, succeeded
    and observations_used); with trace a fifth value, the TRACE array [T]."""
    block, held = packed
    tr = np.zeros(max(held.T, 1), trace_dtype)

    def part(first, count):
        c = np.zeros(len(keys), np.int64)
        rc = fn(sliced(block, first, count), *own, c.ctypes.data, tr.ctypes.data if trace else None)
        assert rc == 0, rc
        return (c,)

    (c,) = total(run_sliced(held.T, part, select, workers), np.zeros(len(keys), np.int64))
    counts = dict(zip(keys, (int(v) for v in c)))
    counts.update(extra)
    counts["succeeded"] = int(((held.points["status"] & 14) == 14).sum())
    counts["observations_used"] = int(held.points["n_views"].sum())
    out = (held.points, held.residuals, held.mask, counts)
    return out + (tr[:held.T],) if trace else out
