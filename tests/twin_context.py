"""_lib.Context's reconstruction surface on the CPU: a class that holds the session state of a context (tracks, point records,
residuals, inlier bytes, pose list, camera, triangulation thresholds and route) and implements the STAGE calls by running the host
twins and references that the stage tests compare the device with.  The glue -- initialize, grow, alternate, reconstruct -- is not
written again: the class borrows the functions of _lib.Context, so the Python under test is the same code on both sides.

Every stage goes through the one handle of tests/twin_host.py.  Test infrastructure only."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import complete_twin
import extend_twin
import filter_twin
import pose_twin
import refine_camera_twin
import refine_points_twin
import refine_poses_twin
import registration_twin
import robust_triangulation_twin
import tracks_ref
import triangulation_twin
import twin_host
import verify_twin
import visibility_twin
from monocularsfm_amd import _lib
from oracle import c_oracle

host = twin_host.load


def _state_error(what):
    return _lib.MsfmError(_lib.E_STATE, what)


class TwinContext:
    # ---- the glue under test: _lib.Context's own functions -------------------------------------------------------------------------------
    initialize = _lib.Context.initialize
    grow = _lib.Context.grow
    alternate = _lib.Context.alternate
    reconstruct = _lib.Context.reconstruct
    poses = _lib.Context.poses
    _kept = _lib.Context._kept

    def __init__(self, device=0):
        self._desc, self._kps = {}, {}
        self._model, self._verify_cam, self._two_view = _lib.VERIFY_FUNDAMENTAL, None, None
        self._session = None            # the track session: dict(ids, min_pair_matches, lists)
        self._tracks = None
        self._records = None            # the two-view records of the last verified call
        self._clear_map()

    def _clear_map(self):
        self._points = self._residuals = self._mask = self._pose_list = self._cam = self._thr = None
        self._registrations = self._pose_refinements = None

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- images, matching, verification --------------------------------------------------------------------------------------------------
    def upload_image(self, image_id, desc):
        self._desc[int(image_id)] = np.ascontiguousarray(desc, np.float32)

    def upload_keypoints(self, image_id, kpts):
        self._kps[int(image_id)] = np.ascontiguousarray(kpts, np.float32)

    def image_rows(self, image_id):
        return len(self._desc[int(image_id)])

    def set_limits(self, max_pairs_per_batch=0, scratch_bytes=0):
        pass                            # (results do not depend on the cuts)

    def set_verification_model(self, model, camera=None):
        if int(model) != _lib.VERIFY_ESSENTIAL:
            raise NotImplementedError("the stand-in verifies under VERIFY_ESSENTIAL only")
        self._model, self._verify_cam = int(model), refine_camera_twin.camera8(camera)

    def set_two_view_geometry(self, enable=True, min_num_inliers=100, tri_max_error=2.0, tri_min_angle=4.0):
        self._two_view = (int(min_num_inliers), float(tri_max_error), float(tri_min_angle)) if enable else None

    def match_pairs(self, pairs, ratio=0.8, cross_check=True, max_distance=0.7, fetch=True):
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        offs, q, t, d = c_oracle.match_pairs(self._desc, pairs, ratio, cross_check, max_distance, nthreads=16)
        out = (offs, np.ascontiguousarray(np.stack([q, t], 1).astype(np.int32)).reshape(-1, 2), d)
        self._fold(pairs, out)
        return out

    def match_pairs_verified(self, pairs, ratio=0.8, cross_check=True, max_distance=0.7, threshold=3.0, confidence=0.99, max_iters=1000,
                             seed=0x5eed5eed, fetch=True):
        """the oracle's lists through the verification twin; with the two-view geometry on, tests/pose_twin.geometry per pair, which
        returns the essential matrix's mask and the record of one and the same run"""
        if self._model != _lib.VERIFY_ESSENTIAL:
            raise NotImplementedError("the stand-in verifies under VERIFY_ESSENTIAL only")
        pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        offs, q, t, d = c_oracle.match_pairs(self._desc, pairs, ratio, cross_check, max_distance, nthreads=16)
        qt = np.ascontiguousarray(np.stack([q, t], 1).astype(np.int32)).reshape(-1, 2)
        kps = {i: k[:, :2] for i, k in self._kps.items()}
        pairs_l = [(int(a), int(b)) for a, b in pairs]
        if self._two_view is None:
            self._records = None
            out = verify_twin.run(host(), (offs, qt, d), pairs_l, kps, 1, self._verify_cam, False, 0.7, threshold, confidence,
                                  int(max_iters), int(seed))["lists"]
        else:
            h = host()

            def one(p):
                i, j = pairs_l[p]
                s, e = offs[p], offs[p + 1]
                return pose_twin.geometry(h, kps[i][qt[s:e, 0]], kps[j][qt[s:e, 1]], self._verify_cam, self._two_view, threshold,
                                          confidence, int(max_iters), int(seed))

            with ThreadPoolExecutor(max_workers=pose_twin.WORKERS) as pool:
                res = list(pool.map(one, range(len(pairs_l))))
            keep = np.concatenate([r[0] for r in res]) if res else np.zeros(0, bool)
            out_off = np.zeros(len(pairs_l) + 1, np.int64)
            out_off[1:] = np.cumsum([int(r[0].sum()) for r in res])
            self._records = np.zeros(len(pairs_l), _lib.TWO_VIEW_RECORD)
            for p, r in enumerate(res):
                self._records[p] = r[1]
            out = (out_off, qt[keep].reshape(-1, 2), d[keep])
        self._fold(pairs, out)
        return out

    def two_view_geometry(self, n_pairs):
        if self._records is None:
            raise _state_error("the last verified call ran without the two-view geometry")
        return self._records[:int(n_pairs)].copy()

    # ---- tracks ----------------------------------------------------------------------------------------------------------------------------
    def tracks_begin(self, ids, min_pair_matches=0, add_only=False):
        ids = [int(i) for i in np.asarray(ids).reshape(-1)]
        self._session = dict(ids=ids, min_pair_matches=int(min_pair_matches), add_only=bool(add_only), lists=[], open=True)
        self._track_ids = list(ids)
        self._tracks = self._track_stats = None
        self._clear_map()

    def _fold(self, pairs, lists):
        s = self._session
        if s is not None and s["open"] and not s["add_only"]:
            s["lists"].append((pairs.copy(), lists[0].copy(), lists[1].copy()))

    def tracks_add(self, pairs, offsets, qt):
        self._session["lists"].append((np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offsets, np.int64), np.asarray(qt, np.int32).reshape(-1, 2)))

    def tracks_finish(self, min_length=2, max_length=0, keep_inconsistent=False):
        s = self._session
        s["open"] = False
        rows = [self.image_rows(i) for i in s["ids"]]
        r = tracks_ref.build(s["ids"], rows, s["lists"], s["min_pair_matches"], int(min_length), int(max_length), bool(keep_inconsistent))
        self._tracks = (r["offsets"], r["image_ids"], r["point_idx"], r["consistent"])
        self._track_of = r["track_ids"]
        self._track_stats = dict(r["stats"])
        self._clear_map()
        return dict(self._track_stats)

    def tracks(self):
        return tuple(a.copy() for a in self._tracks)

    def track_ids(self, image_id):
        return self._track_of[int(image_id)].copy()

    def tracks_end(self):
        self._session = self._tracks = self._track_stats = None
        self._clear_map()

    # ---- the map ---------------------------------------------------------------------------------------------------------------------------
    def _need_map(self):
        if self._points is None:
            raise _state_error("no triangulated points")

    def _common(self):
        """(tracks, declared ids, keypoints) as every twin driver takes them"""
        return self._tracks, self._session["ids"], self._kps

    def triangulate_tracks(self, camera, poses, max_error=2.0, min_angle=1.5, min_views=2, robust=False, max_hypotheses=64):
        cam = refine_camera_twin.camera8(camera)
        lst = _lib.pose_table(poses)
        self._tri_route = int(max_hypotheses) if robust else 0
        self._tri_thresholds = (float(max_error), float(min_angle))
        thr = (float(max_error), float(min_angle), int(min_views))
        extra = {}
        if robust:
            pts, res, mask, extra = robust_triangulation_twin.run(host(), *self._common(), lst, cam, thr + (int(max_hypotheses),))
        else:
            pts, res = triangulation_twin.run(host(), *self._common(), lst, cam, thr)
            mask = None
        self._clear_map()
        self._points, self._residuals, self._mask, self._pose_list, self._cam, self._thr = pts, res, mask, lst, cam, thr
        out = dict(triangulation_twin.counts(pts), tracks=len(pts))
        out.update(extra)
        return out

    def points3d(self):
        self._need_map()
        return self._points.copy(), self._residuals.copy()

    def point_inliers(self):
        self._need_map()
        if self._mask is None:
            raise _state_error("the session has no inlier bytes")
        return self._mask.copy()

    def pose_list(self):
        self._need_map()
        return self._pose_list[0].copy(), self._pose_list[1].copy()

    def camera(self):
        self._need_map()
        return dict(zip(("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"), self._cam))

    def _changed(self):
        self._registrations = self._pose_refinements = None

    def register_images(self, camera, image_ids, max_error=4.0, confidence=0.9999, max_iters=1024, min_inliers=15, refine_iters=10):
        self._need_map()
        ids = [int(i) for i in np.asarray(image_ids).reshape(-1)]
        got = registration_twin.run(host(), self._tracks, self._points, ids, self._kps, refine_camera_twin.camera8(camera),
                                    max_error=max_error, confidence=confidence, max_iters=max_iters, min_inliers=min_inliers,
                                    refine_iters=refine_iters)
        self._registrations = got
        rec = got[0]
        rounds, solved = registration_twin.schedule(rec, max_iters)
        return dict(images=len(ids), attempted=int(((rec["status"] & _lib.REG_ATTEMPTED) != 0).sum()), succeeded=int(_lib.registered(rec).sum()),
                    rounds=rounds, hypotheses=solved, correspondences=len(got[2]))

    def registrations(self):
        if self._registrations is None:
            raise _state_error("no registrations")
        return tuple(a.copy() for a in self._registrations)

    def extend_points(self, poses, max_hypotheses=None):
        self._need_map()
        if max_hypotheses is None:
            max_hypotheses = getattr(self, "_tri_route", 0)
        pts, res, mask, counts, lst = extend_twin.run(host(), *self._common(), self._pose_list, _lib.pose_table(poses), self._cam,
                                                      self._points, self._residuals, self._mask, self._thr, int(max_hypotheses))
        self._points, self._residuals, self._mask, self._pose_list = pts, res, mask, lst
        self._changed()
        return counts

    def refine_points(self, max_iters=10, step_tol=1e-10):
        self._need_map()
        pts, res, counts = refine_points_twin.run(host(), *self._common(), self._pose_list, self._cam, self._points, self._residuals,
                                                  self._mask, self._thr[:2], (int(max_iters), float(step_tol)))
        self._points, self._residuals = pts.copy(), res.copy()
        self._changed()
        return counts

    def refine_poses(self, max_iters=10, step_tol=1e-6, min_observations=15, fixed=()):
        self._need_map()
        pts, res, lst, rec, counts = refine_poses_twin.run(host(), *self._common(), self._pose_list, self._cam, self._points,
                                                           self._residuals, self._mask, self._thr[:2],
                                                           (int(max_iters), float(step_tol), int(min_observations)), [int(i) for i in fixed])
        self._points, self._residuals, self._pose_list = pts.copy(), res.copy(), (lst[0].copy(), lst[1].copy())
        self._changed()
        self._pose_refinements = rec.copy()
        return counts

    def pose_refinements(self):
        if self._pose_refinements is None:
            raise _state_error("no pose refinements")
        return self._pose_refinements.copy()

    def refine_camera(self, mask=("fx_fy",), max_iters=10, step_tol=1e-6, min_observations=100):
        self._need_map()
        before = self.camera()
        pts, res, cam, counts = refine_camera_twin.run(host(), *self._common(), self._pose_list, self._cam, self._points,
                                                       self._residuals, self._mask, self._thr[:2],
                                                       (int(max_iters), float(step_tol), int(min_observations)), _lib.camera_mask(mask))
        self._points, self._residuals, self._cam = pts.copy(), res.copy(), tuple(cam)
        self._changed()
        return dict(counts, camera_before=before, camera_after=self.camera())

    def filter_points(self, max_error=None, min_angle=None, image_ids=None):
        self._need_map()
        params = (float(max_error), float(min_angle)) if max_error is not None and min_angle is not None else None
        pts, res, mask, counts = filter_twin.run(host(), *self._common(), self._pose_list, self._cam, self._points, self._residuals,
                                                 self._mask, self._thr[:2], params, list(image_ids) if image_ids is not None else ())
        self._points, self._residuals, self._mask = pts, res, mask
        self._changed()
        return counts

    def complete_points(self, max_error=None, image_ids=None):
        self._need_map()
        pts, res, mask, counts = complete_twin.run(host(), *self._common(), self._pose_list, self._cam, self._points,
                                                   self._residuals, self._mask, self._thr[:2], max_error,
                                                   list(image_ids) if image_ids is not None else ())
        self._points, self._residuals, self._mask = pts, res, mask
        self._changed()
        return counts

    def visibility(self, query=(), basis="map", route="auto"):
        if self._tracks is None:
            raise _state_error("no finished tracks")
        if basis == "map":
            self._need_map()
        on_map = basis == "map"
        rec, mat, counts = visibility_twin.run(host(), self._tracks, self._session["ids"], self._pose_list if on_map else None,
                                               self._points if on_map else None, self._mask if on_map else None,
                                               [int(i) for i in query], basis)
        flags = rec["flags"]
        counts = dict(counts, images=len(rec), query=len(mat), posed=int(((flags & _lib.VIS_POSED) != 0).sum()))
        return rec, mat, counts
