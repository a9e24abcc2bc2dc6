"""Independent numpy reference of the map visibility (include/msfm_match.h "map visibility"): written from the definitions, not from
csrc/msfm_visibility.h's walk -- boolean tracks x images incidence matrices and their products.  Test infrastructure only."""
import numpy as np

from monocularsfm_amd import _lib

OK = _lib.TRI_POINT | _lib.TRI_ERROR_OK | _lib.TRI_ANGLE_OK


def posed_ids(pose_list):
    """The ids with a valid pose of a dict id -> (R, t) / None or an (ids, POSE_RT) pair; None -> empty."""
    if pose_list is None:
        return set()
    if isinstance(pose_list, dict):
        return {int(i) for i, p in pose_list.items() if p is not None}
    ids, tab = pose_list
    return {int(i) for i, p in zip(ids, tab) if p["valid"]}


def run(tracks, ids, pose_list=None, points=None, mask=None, query=(), basis="map"):
    """The arguments of visibility_twin.run -> (VISIBILITY array [n], matrix uint32 [len(query), n], dict of the three counters)."""
    offsets, img = np.asarray(tracks[0], np.int64), np.asarray(tracks[1], np.int64)
    cons = np.asarray(tracks[3]) != 0
    ids = np.asarray(sorted(int(i) for i in ids), np.int64)
    T, n = len(offsets) - 1, len(ids)
    col = np.searchsorted(ids, img)                              # every element's image as a column
    trk = np.repeat(np.arange(T), np.diff(offsets))              # ... and its track as a row
    have = np.zeros((T, n), bool)                                # the track has an element in the image
    have[trk, col] = True
    if basis == "tracks":
        standing = cons.copy()
        posed = np.zeros(n, bool)
        fit = have.copy()
    else:
        standing = cons & ((np.asarray(points["status"][:T]) & OK) == OK)
        posed = np.isin(ids, sorted(posed_ids(pose_list)))
        fit = np.zeros((T, n), bool)
        fit[trk, col] = True if mask is None else (np.asarray(mask[:len(img)]) != 0)
    counts = have & standing[:, None] & (fit | ~posed[None, :])  # the counting elements
    rec = np.zeros(n, _lib.VISIBILITY)
    rec["image_id"] = ids
    rec["flags"] = np.where(posed, _lib.VIS_POSED, 0) | np.where(np.isin(ids, [int(i) for i in query]), _lib.VIS_QUERIED, 0)
    rec["n_elements"] = (have & cons[:, None]).sum(axis=0)
    rec["n_visible"] = (have & standing[:, None]).sum(axis=0)
    rec["n_points"] = np.where(posed, counts.sum(axis=0), 0)
    rows = np.searchsorted(ids, np.asarray([int(i) for i in query], np.int64))
    c64 = counts.astype(np.int64)
    mat = (c64[:, rows].T @ c64).astype(np.uint32).reshape(len(rows), n)
    return rec, mat, {"tracks_counted": int(standing.sum()), "elements_counted": int(counts.sum()), "pair_increments": int(mat.sum(dtype=np.int64))}
