"""Inputs shared by the map extension's CPU and GPU tests: ring scenes (tests/refine_poses_fixtures.chosen_scene) in which the images
posed at the triangulation leave some tracks standing (they are continued), some with a point below min_angle, some failing the error
test and some never attempted (they are created), with planted outliers in old and in new images; the increments the rest of the
images arrive in.  Test infrastructure only.

Seeds tried on the CPU for the reference cases (tests/test_extend_points_reference.py): scene seeds 3, 5 and 11 with 0.3 px of noise.
The independent reference leaves out no track under any of them (no new observation's error within 1e-6 px of max_error, no scanned
angle within 1e-6 degrees of min_angle); seed 3 is used.  Smallest margins found: DESIGN.md section 20."""
import numpy as np

import refine_poses_fixtures as pfx

CAM = pfx.CAM
CAM_D = (2500.0, 2450.0, 1536.0, 1152.0, -0.02, 0.005, 2e-4, -1e-4)   # distortion and fx != fy (the keypoints are CAM's: errors of some px)
THRESHOLDS = (2.0, 1.5, 2)           # the reference's Triangulator::Parameters
THRESHOLDS_D = (40.0, 1.0, 2)
T = 96
N_IMG = 10
# image position -> the tracks it sees (images 0 and 1 see every track: refine_poses_fixtures.membership)
SIZES = [T, T, 80, 64, list(range(16, 88)), list(range(8, 90)), list(range(0, T, 2)), 48, list(range(40, T)), T]
FIRST = (1, 2, 3)                    # positions posed at the triangulation: tracks 0 .. 63 stand (2.4 degrees), 64 .. 79 have a point
#                                      below min_angle (1.2 degrees), 80 .. 95 have one posed view and are not attempted
ONE = [(0, 4, 5, 6, 7, 8, 9)]        # the rest in one increment ...
TWO = [(4, 5), (0, 6, 7, 8, 9)]      # ... and in two: the first leaves the tracks 0 .. 7 and 90 .. 95 untouched, the second creates 90 .. 95
# (track, image position, dx): 30 px off -- in a new image of a standing track: rejected by error; in an image posed at the
# triangulation: the track fails ERROR_OK there, is created by the extension and retried on the robust route
OUTLIERS = [(20, 4, 30.0), (24, 5, -30.0), (21, 9, 30.0), (10, 2, 30.0), (33, 3, -30.0), (70, 2, 30.0)]


def scene(seed=3, noise_px=0.3, sizes=SIZES, outliers=OUTLIERS, n_tracks=T):
    """-> (ids, kps list, true poses, tracks)"""
    ids, kps, poses, seen = pfx.chosen_scene(pfx.general_points(n_tracks, seed + 50), sizes, noise_px=noise_px, seed=seed)
    for t, i, dx in outliers:
        assert seen[t, i]
        kps[i][t, 0] += np.float32(dx)
    return ids, kps, poses, pfx.tracks_of(seen, ids), seen


def some(poses, ids, positions):
    return {int(ids[p]): poses[int(ids[p])] for p in positions}
