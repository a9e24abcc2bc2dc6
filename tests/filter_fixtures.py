"""Inputs shared by the map filtering's CPU and GPU tests: the states the filter is run on -- the extension's ring scene
(tests/extend_fixtures.scene) after the plain twin under a loose session, after the pose refinement twin from perturbed poses, after
the robust twin extended in two increments, under a distorted camera -- and one generated group with what that scene lacks (GROUP
below).  Every state is (tracks, ids, kps, camera, session thresholds, pose list, points, residuals, inlier bytes or None) plus the
call's parameters and scope.  Test infrastructure only.

Seeds tried on the CPU for the reference cases (tests/test_filter_points_reference.py): scene seeds 3, 5 and 11.  The independent
reference leaves out no track under any of them (no error within 1e-6 px of a threshold it was compared with, no scanned angle within
1e-6 degrees of one); seed 3 is committed.  Smallest margins found: DESIGN.md section 22."""
import numpy as np

import extend_fixtures as efx
import extend_twin as etw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import robust_triangulation_twin as robtw
import triangulation_twin as tw

CAM = efx.CAM
LOOSE = (40.0, 1.0, 2)               # a session that admits the scene's 30 px outliers into standing points
TIGHT = (2.0, 1.5)                   # the reference's Triangulator::Parameters, as the call's thresholds
# case B: refine_poses_fixtures' route "lost_and_gained" (twelve ring cameras, 120 tracks, 8 px of noise, a (12 px, 3 degree) session):
# the one committed job in which the pose refinement's re-verdict takes ERROR_OK from points (2 lost, 4 gained).  It has its own seeds.
B_ROUTE = "lost_and_gained"

# ---- the generated group ----------------------------------------------------------------------------------------------------------------
# Ten ring cameras (1.2 degrees between neighbours), 24 tracks, 0.05 px of noise; image 5 is TURNED (below) and seen by 12 .. 15 only.
#    0 ..  3   2 views (0, 1).  0, 1: 30 px off in y in image 1 -> both errors ~15 px: removed by views.  2, 3: clean, 1.2 degrees:
#              removed by angle under a call with min_angle 1.5 without a drop.
#    4 ..  7   3 views (0, 1, 2).  4, 5: two bad observations (30 px in image 1, -30 px in image 2): removed by views.
#    8 .. 11   3 views (0, 1, 9).  8, 9: 4.5 px off in y in image 9 -> its error ~3 px, the others' ~1.5 px: the dropped view was the
#              only wide pair, images 0 and 1 are 1.2 degrees apart: removed by angle after a drop.
#   12 .. 15   6 views (0, 1, 3, 4, 5, 6).  Image 5 is turned: dropped by depth, trimmed.  13: 6 px off in y in image 3 as well: both
#              kinds of drop in one track.
#   16 .. 19   8 views (0, 1, 2, 3, 4, 6, 7, 8).  16, 17: 4 px off in y in image 4 -> its error ~3.5 px, the others' ~0.5 px: under a
#              (2 px, 1.5 degree) session the point lacks ERROR_OK and a trim with NULL parameters regains it.
#   20 .. 23   9 views (all but 5), clean: untouched.
GROUP_T = 24
GROUP_SIZES = [GROUP_T, GROUP_T, list(range(4, 8)) + list(range(16, 24)), list(range(12, 24)), list(range(12, 24)), list(range(12, 16)),
               list(range(12, 24)), list(range(16, 24)), list(range(16, 24)), list(range(8, 12)) + list(range(20, 24))]
GROUP_MOVED = [(0, 1, 30.0), (1, 1, 30.0), (4, 1, 30.0), (4, 2, -30.0), (5, 1, 30.0), (5, 2, -30.0), (8, 9, 4.5), (9, 9, 4.5), (13, 3, 6.0),
               (16, 4, 4.0), (17, 4, 4.0)]       # (track, image position, dy)
GROUP_TURNED = 5
GROUP_NOISE = 0.05


def turned(pose):
    """the camera turned by 180 degrees about its own y axis: every point that was in front of it is behind it"""
    D = np.diag([-1.0, 1.0, -1.0])
    return D @ np.asarray(pose[0], np.float64), D @ np.asarray(pose[1], np.float64)


def turn_image(kps, poses, ids, position, cam=CAM):
    """Image `position` turned, its keypoints mirrored about cy: (x, y) under the turned camera is the projection THROUGH the centre of
    the same 3-D point (the DLT's rows are the same up to sign), so the point triangulates with small errors and a negative depth."""
    kps[position][:, 1] = (np.float32(2.0 * cam[3]) - kps[position][:, 1]).astype(np.float32)
    poses[int(ids[position])] = turned(poses[int(ids[position])])


def group_scene(seed=3):
    """-> (ids, kps list, poses (image GROUP_TURNED turned), tracks)"""
    ids, kps, poses, seen = pfx.chosen_scene(pfx.general_points(GROUP_T, seed + 50), GROUP_SIZES, noise_px=GROUP_NOISE, seed=seed)
    for t, i, dy in GROUP_MOVED:
        assert seen[t, i]
        kps[i][t, 1] += np.float32(dy)
    poses = dict(poses)
    turn_image(kps, poses, ids, GROUP_TURNED)
    return ids, kps, poses, pfx.tracks_of(seen, ids)


def state(tracks, ids, kps, cam, thr, lst, pp, pr, pm, params=None, scope=()):
    return dict(tracks=tracks, ids=ids, kps=kps, cam=cam, thr=thr, lst=lst, before=(pp, pr, pm), params=params, scope=tuple(scope))


def case_a(host, seed=3):
    """the plain twin under a loose session: standing points hold the scene's outliers; filtered at (2.0, 1.5)"""
    ids, kps, poses, tracks, _ = efx.scene(seed)
    pp, pr = tw.run(host, tracks, ids, kps, poses, CAM, LOOSE)
    return state(tracks, ids, kps, CAM, LOOSE, poses, pp, pr, None, TIGHT)


def case_b(host, seed=3):
    """the pose refinement twin from perturbed poses: REPOSED records, some lost; NULL parameters"""
    ids, kps, start, seen, fixed, thr, _ = pfx.route_case(B_ROUTE)
    tracks, pp, pr = pfx.first_records(host, ids, kps, start, seen, thr, pfx.CAM)
    pp, pr, lst, _, cnt = ptw.run(host, tracks, ids, kps, start, pfx.CAM, pp, pr, None, thr, pfx.ROUTE_PARAMS, fixed=fixed)
    out = state(tracks, ids, kps, pfx.CAM, thr + (2,), lst, pp, pr, None)
    out["pose_counts"] = cnt
    return out


def case_c(host, seed=3, params=None):
    """the robust session, extended in two increments; scoped to the last increment's images"""
    ids, kps, poses, tracks, _ = efx.scene(seed)
    thr, mh = efx.THRESHOLDS, 64
    lst = efx.some(poses, ids, efx.FIRST)
    pp, pr, pm, _ = robtw.run(host, tracks, ids, kps, lst, CAM, thr + (mh,))
    for inc in efx.TWO:
        pp, pr, pm, _, lst = etw.run(host, tracks, ids, kps, lst, efx.some(poses, ids, inc), CAM, pp, pr, pm, thr, mh)
    return state(tracks, ids, kps, CAM, thr, lst, pp, pr, pm, params, [int(ids[p]) for p in efx.TWO[-1]])


def case_d(host, seed=3):
    """the distorted camera with fx != fy under its loose session (the keypoints are CAM's: errors of some px); filtered at (6.0, 1.5)"""
    ids, kps, poses, tracks, _ = efx.scene(seed)
    pp, pr = tw.run(host, tracks, ids, kps, poses, efx.CAM_D, efx.THRESHOLDS_D)
    return state(tracks, ids, kps, efx.CAM_D, efx.THRESHOLDS_D, poses, pp, pr, None, (6.0, 1.5))


def case_group(host, seed=3, loose=True):
    """the generated group: under the loose session filtered at (2.0, 1.5), or under a (2.0, 1.5) session with NULL parameters"""
    ids, kps, poses, tracks = group_scene(seed)
    thr = LOOSE if loose else TIGHT + (2,)
    pp, pr = tw.run(host, tracks, ids, kps, poses, CAM, thr)
    return state(tracks, ids, kps, CAM, thr, poses, pp, pr, None, TIGHT if loose else None)


CASES = {
    "A_loose_plain": case_a,
    "B_reposed_null": case_b,
    "C_robust_extended_scoped": case_c,
    "C_robust_extended_scoped_tight": lambda host, seed=3: case_c(host, seed, (1.0, 2.5)),
    "D_distorted": case_d,
    "G_group_loose": case_group,
    "G_group_null": lambda host, seed=3: case_group(host, seed, False),
}


def poses_dict(lst):
    """a pose list in either form -> dict id -> (R, t) / None"""
    if isinstance(lst, dict):
        return dict(lst)
    return ptw.poses_dict(*lst)
