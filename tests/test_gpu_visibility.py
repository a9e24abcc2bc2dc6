"""Map visibility on the device (msfm_map_visibility, csrc/msfm_visibility.hip.h) against the host twin (csrc/msfm_visibility.h,
MapVisibility, through tests/visibility_twin.py): records, matrix and counters BYTE FOR BYTE, under MSFM_VIS_ROUTE_GLOBAL and
MSFM_VIS_ROUTE_LDS forced and under AUTO -- all three must give the same bytes.  The twin is fed the device's own state (tracks(),
points3d(), point_inliers() where they exist, pose_list()), which the earlier GPU tests hold equal to their twins; every comparison
is followed by a comparison of the session's state with what it was: the call is read-only.  The twin itself is checked against an
independent numpy reference in tests/test_visibility_reference.py.  Then the glue built on the counts: initialize, grow(max_images=,
window=), reconstruct."""
import ctypes as C

import numpy as np
import pytest

import extend_fixtures as efx
import refine_poses_fixtures as pfx
import visibility_ref as vref
import visibility_twin as vtw
from monocularsfm_amd import _lib
from test_gpu_complete_points import plant
from test_gpu_extend_points import code, same_state, some, state
from test_gpu_robust_triangulation import open_ring, ring_job, second_pass_job

pytestmark = pytest.mark.gpu
CAM = efx.CAM
THR = efx.THRESHOLDS
ROUTES = (("global", _lib.VIS_ROUTE_GLOBAL), ("lds", _lib.VIS_ROUTE_LDS), ("auto", None))


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return vtw.load_host()


def vis_same(ctx, host, tracks, ids, query=(), basis="map"):
    """msfm_map_visibility under the three routes against the twin run from the session's state, which no call changes
    -> (records, matrix, the last stats)"""
    before = state(ctx) if basis == "map" else None
    p0, _, m0, lst0 = before if before else (None, None, None, None)
    wr, wm, wc = vtw.run(host, tracks, ids, lst0, p0, m0, query, basis)
    for name, ran in ROUTES:
        rec, mat, st = ctx.visibility(query, basis, name)
        assert rec.tobytes() == wr.tobytes(), (name, np.nonzero(rec != wr)[0][:8])
        assert mat.shape == wm.shape and mat.tobytes() == wm.tobytes(), (name, np.argwhere(mat != wm)[:8])
        assert {k: st[k] for k in vtw.COUNT_KEYS} == wc, (name, st, wc)
        assert st["route"] == ran if ran else st["route"] in (_lib.VIS_ROUTE_GLOBAL, _lib.VIS_ROUTE_LDS)
        assert (st["images"], st["query"]) == (len(ids), len(query)) and st["visibility_ms"] >= 0.0 and st["device_bytes"] > 0
        assert st["posed"] == int(((rec["flags"] & _lib.VIS_POSED) != 0).sum())
        if before:
            assert same_state(before, state(ctx)), name
    return rec, mat, st


def every_form(ctx, host, tracks, ids, basis="map"):
    """n_query = 0, 1 and n"""
    ids = [int(i) for i in ids]
    vis_same(ctx, host, tracks, ids, (), basis)
    vis_same(ctx, host, tracks, ids, ids[-1:], basis)
    return vis_same(ctx, host, tracks, ids, ids[::-1], basis)


# ---- track counts: the wave, block and grid-stride edges of vis_lane_kernel ------------------------------------------------------------
def test_track_counts_at_the_wave_and_block_edges(tctx, host):
    """T = 1, 63, 64, 65, 255, 256, 257 kept tracks; the tracks at the lanes 0, 63 | 64, 255 | 256 have length 5, every other length 3;
    image 0 is in every track (the hot counter: its counts are T exactly); images 3 and 4 have no pose."""
    for T in (257, 256, 255, 65, 64, 63, 1):
        lengths = [5 if j in (0, 63, 64, 255, 256) else 3 for j in range(T)]
        ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
        assert open_ring(tctx, ids, kps, lst, T)["tracks_kept"] == T
        tracks = tctx.tracks()
        rec, mat, st = every_form(tctx, host, tracks, ids, "tracks")
        assert rec["n_elements"][0] == T == st["tracks_counted"] and st["elements_counted"] == int(tracks[0][-1])
        tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2)), *THR)
        rec, mat, st = every_form(tctx, host, tracks, ids)
        assert rec["n_points"][0] == rec["n_visible"][0] == st["tracks_counted"] > 0 and st["posed"] == 3
        assert rec["n_points"][3] == 0 and rec["n_visible"][3] == min(T, len([j for j in (0, 63, 64, 255, 256) if j < T]))
        tctx.tracks_end()


def test_second_grid_stride_pass(tctx, host):
    """vis_lane_kernel<false>'s grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run a second pass of the
    wave-uniform t0 loop; the LDS route's 2 x CUs workgroups run many.  Tracks of length 3 over triples of images."""
    cus = tctx.device_info()["cu_count"]
    T = 8 * 256 * cus + 8192
    ids, kps, poses, lists = second_pass_job(T)
    d = np.random.default_rng(1).integers(0, 256, (8192, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    for l in lists:
        tctx.tracks_add(*l)
    assert tctx.tracks_finish()["tracks_kept"] == T
    tracks = tctx.tracks()
    ids = [int(i) for i in ids]
    rec, mat, st = vis_same(tctx, host, tracks, ids, ids[-3:], "tracks")
    assert st["tracks_counted"] == T and st["elements_counted"] == 3 * T and mat[0, -1] == mat[2, -1] == rec["n_elements"][-1]
    _, full, st = vis_same(tctx, host, tracks, ids, ids, "tracks")   # (195 x 195 words: the LDS route keeps the matrix in global memory)
    assert st["pair_increments"] == 9 * T and np.array_equal(full[-3:], mat)
    tctx.triangulate_tracks(CAM, {i: p for i, p in poses.items() if i != ids[-1]}, 60.0, 1.0, 2)
    rec, mat, st = vis_same(tctx, host, tracks, ids, [ids[0], ids[-1]])
    assert st["tracks_counted"] > T // 2 and rec["n_points"][-1] == 0 and rec["n_visible"][-1] == mat[1, -1] > 0
    tctx.tracks_end()


# ---- declared images and track lengths: the lane path, the wave path and the threshold between them -------------------------------------
@pytest.mark.parametrize("lengths", ([2] * 5, [3, 2, 3, 3, 2], [65, 64, 2, 3, 65, 64, 2]), ids=("n2", "n3", "n65"))
def test_declared_image_counts(tctx, host, lengths):
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
    assert len(ids) == max(lengths)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    every_form(tctx, host, tracks, ids, "tracks")
    tctx.triangulate_tracks(CAM, poses, 2.0, 1.0, 2)
    rec, mat, st = every_form(tctx, host, tracks, ids)
    assert st["tracks_counted"] == len(lengths) and st["pair_increments"] == sum(n * n for n in lengths)
    tctx.tracks_end()


@pytest.mark.parametrize("robust", (False, True))
def test_tracks_longer_than_a_wave(tctx, host, robust):
    """A ring of 72 images: tracks of 2, 3, 63, 64 (one lane each) and 65, 66, 70, 72 elements (vis_wave_kernel: one wave each; the
    72-element track gives lanes 0 .. 7 two elements), twice, with a 40 px outlier in a long and in a short track on the robust
    session.  The matrix of every image: 72 rows."""
    lengths = [72, 64, 65, 2, 70, 3, 63, 66] * 2
    ids, kps, poses, lst = ring_job(lengths, outlier={0: 40, 5: 1, 10: 64} if robust else None, noise_px=0.1)
    st0 = open_ring(tctx, ids, kps, lst, len(lengths))
    assert st0["longest_track"] == 72 and len(ids) == 72
    tracks = tctx.tracks()
    every_form(tctx, host, tracks, ids, "tracks")
    tctx.triangulate_tracks(CAM, {i: p for i, p in poses.items() if i not in (int(ids[7]), int(ids[69]))}, 2.0, 1.0, 2, robust=robust,
                            max_hypotheses=16)
    rec, mat, st = every_form(tctx, host, tracks, ids)
    assert st["tracks_counted"] >= len(lengths) - 3 and st["posed"] == 70
    if robust:
        m = tctx.point_inliers()
        assert m[tracks[0][0] + 40] == 0 and rec["n_points"][40] < rec["n_visible"][40]
    tctx.tracks_end()


def test_hot_counter(tctx, host):
    """6000 tracks that all run through the images 0, 1 and 2: every lane of every wave adds to the same three words of each
    per-image counter and, with those images queried, to the same cells.  Counts are exact under contention."""
    lengths = [3, 4, 5, 6] * 1500
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    ids = [int(i) for i in ids]
    rec, mat, st = vis_same(tctx, host, tracks, ids, ids[:3], "tracks")
    assert np.all(rec["n_elements"][:3] == 6000) and np.all(mat[:, :3] == 6000) and st["pair_increments"] == 3 * 27000
    tctx.triangulate_tracks(CAM, poses, 2.0, 1.0, 2)
    rec, mat, st = vis_same(tctx, host, tracks, ids, ids[:3])
    assert rec["n_points"][0] == st["tracks_counted"] == mat[1, 0] > 5000
    tctx.tracks_end()


# ---- the forms of the call -------------------------------------------------------------------------------------------------------------
def raw(ctx, query, basis, route, images=True, matrix=True):
    """the C call with out_images and / or out_covisible NULL"""
    q = np.ascontiguousarray(query, np.int32)
    n = len(ctx._track_ids)
    rec, mat, st = np.zeros(max(n, 1), _lib.VISIBILITY), np.full((len(q), n), 7, np.uint32), _lib.VisibilityStats()
    prm = _lib.VisibilityParams(basis, route)
    rc = ctx._L.msfm_map_visibility(ctx._h, C.byref(prm), q.ctypes.data_as(C.POINTER(C.c_int32)) if len(q) else None, len(q),
                                    rec.ctypes.data if images else None, mat.ctypes.data if matrix else None, C.byref(st))
    assert rc == 0, ctx._L.msfm_last_error(ctx._h)
    return rec[:n], mat, _lib._dict(st)


def test_query_forms(tctx, host):
    """n_query = 0 with a NULL matrix; NULL out_images with a matrix; NULL parameters; a query image without a pose; a query image
    that no track sees (an all-zero row and column); a permuted query list permutes the rows."""
    lengths = [6, 5, 4, 3, 2, 6]
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
    lone = 1000
    open_ring(tctx, list(ids) + [lone], kps + [kps[0]], lst, len(lengths))
    all_ids = [int(i) for i in ids] + [lone]
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2, 3)), 2.0, 1.0, 2)
    before = state(tctx)
    unposed = int(ids[4])
    rec, mat, st = vis_same(tctx, host, tracks, all_ids, [lone, unposed, int(ids[0])])
    assert not mat[0].any() and not mat[:, -1].any() and rec[-1]["flags"] == _lib.VIS_QUERIED and rec[-1]["n_elements"] == 0
    assert rec[4]["flags"] == _lib.VIS_QUERIED and mat[1, 4] == rec[4]["n_visible"] > 0 and rec[4]["n_points"] == 0
    rec2, mat2, _ = vis_same(tctx, host, tracks, all_ids, [int(ids[0]), lone, unposed])
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(mat2, mat[[2, 0, 1]])
    for route in (_lib.VIS_ROUTE_GLOBAL, _lib.VIS_ROUTE_LDS, _lib.VIS_ROUTE_AUTO):
        r0, _, s0 = raw(tctx, [], _lib.VIS_MAP, route, matrix=False)
        assert np.array_equal(r0["n_visible"], rec["n_visible"]) and s0["pair_increments"] == 0 and s0["query"] == 0
        _, m1, s1 = raw(tctx, [lone, unposed, int(ids[0])], _lib.VIS_MAP, route, images=False)
        assert m1.tobytes() == mat.tobytes() and s1["pair_increments"] == st["pair_increments"]
        raw(tctx, [unposed], _lib.VIS_MAP, route, images=False, matrix=False)
    s = _lib.VisibilityStats()
    assert tctx._L.msfm_map_visibility(tctx._h, None, None, 0, None, None, C.byref(s)) == 0   # NULL parameters: {MAP, AUTO}
    assert s.tracks_counted == st["tracks_counted"] and s.posed == 4
    assert same_state(before, state(tctx))
    tctx.tracks_end()


def test_basis_tracks_straight_after_tracks_finish(tctx, host):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    rec, mat, st = every_form(tctx, host, tracks, ids, "tracks")
    assert np.array_equal(rec["n_elements"], seen.sum(axis=0)) and st["posed"] == 0 and not rec["flags"][0] & _lib.VIS_POSED
    assert np.array_equal(mat[::-1], (seen.T.astype(np.int64) @ seen.astype(np.int64)).astype(np.uint32))
    assert code(tctx.visibility) == _lib.E_STATE and code(tctx.points3d) == _lib.E_STATE   # basis MAP: no points yet
    tctx.tracks_end()


def test_basis_map_after_each_map_call(tctx, host):
    """the extension's scene: after a plain triangulation (no bytes), a robust one, extend_points with rejected observations,
    filter_points that trimmed and removed (planted through API calls alone), complete_points"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR)
    assert code(tctx.point_inliers) == _lib.E_STATE
    rec, _, st = every_form(tctx, host, tracks, ids)
    assert code(tctx.point_inliers) == _lib.E_STATE and st["posed"] == 3   # (as before the call: no bytes)
    posed = (rec["flags"] & _lib.VIS_POSED) != 0
    assert np.array_equal(rec["n_points"][posed], rec["n_visible"][posed])
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
    rec, _, _ = every_form(tctx, host, tracks, ids)
    assert np.any(rec["n_points"][posed] < rec["n_visible"][posed])   # (the hypotheses rejected the planted outliers)
    est = tctx.extend_points(some(poses, ids, efx.TWO[0]))
    assert est["observations_rejected"] > 0
    rec, _, st = every_form(tctx, host, tracks, ids)
    assert st["posed"] == 5
    # (track 1 is seen by the posed images 1, 2 and 3 only: without two of them it is removed)
    fst, kps2 = plant(tctx, ids, kps, [(30, 2), (31, 3), (40, 4), (1, 2), (1, 3)])
    assert fst["trimmed"] >= 3 and fst["removed_by_angle"] + fst["removed_by_views"] > 0
    rec_f, _, st_f = every_form(tctx, host, tracks, ids)
    assert st_f["tracks_counted"] < st["tracks_counted"]
    cst = tctx.complete_points()
    assert cst["admitted"] >= 3
    rec_c, _, st_c = every_form(tctx, host, tracks, ids)
    assert st_c["elements_counted"] == st_f["elements_counted"] + cst["admitted"] and st_c["tracks_counted"] == st_f["tracks_counted"]
    tctx.tracks_end()


def test_inconsistent_tracks_change_no_counter(tctx, host):
    """keep_inconsistent=True: one extra match joins row 1 of image 0 with row 0 of image 1, so the tracks 0 and 1 become one
    inconsistent track.  It is kept, and counts nothing: the records, the matrix and the counters are those of the session finished
    without it."""
    lengths = [5, 4, 6, 3, 2, 6]
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
    d = np.random.default_rng(1).integers(0, 256, (len(lengths), 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(*lst)
    tctx.tracks_add(np.asarray([[ids[0], ids[1]]], np.int32), np.asarray([0, 1], np.int64), np.asarray([[1, 0]], np.int32))
    out = {}
    for keep in (True, False):
        st = tctx.tracks_finish(keep_inconsistent=keep)
        assert st["tracks_kept"] == (5 if keep else 4) and st["tracks_inconsistent"] == 1
        tracks = tctx.tracks()
        assert (tracks[3] == 0).sum() == (1 if keep else 0)
        a = every_form(tctx, host, tracks, ids, "tracks")
        tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2, 3)), 2.0, 1.0, 2)
        b = every_form(tctx, host, tracks, ids)
        out[keep] = [x.tobytes() for x in a[:2] + b[:2]] + [{k: s[k] for k in vtw.COUNT_KEYS} for s in (a[2], b[2])]
    assert out[True] == out[False]
    tctx.tracks_end()


# ---- read-only ---------------------------------------------------------------------------------------------------------------------------
def test_read_only_between_registration_and_fetch(tctx, host):
    """register_images, then visibility, then registrations(): the same bytes as without it; the listed unposed images' n_visible is
    the registration's n_correspondences (an independent kernel's count); pose_refinements() is still fetchable behind refine_poses +
    visibility."""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
    rest = [int(ids[p]) for p in range(len(ids)) if p not in efx.FIRST]
    tctx.register_images(CAM, rest)
    want = [a.tobytes() for a in tctx.registrations()]
    tctx.register_images(CAM, rest)
    rec, mat, _ = every_form(tctx, host, tracks, ids)
    got = tctx.registrations()
    assert [a.tobytes() for a in got] == want
    at = {int(r["image_id"]): k for k, r in enumerate(rec)}
    assert [int(rec["n_visible"][at[i]]) for i in rest] == [int(r["n_correspondences"]) for r in got[0]]
    tctx.refine_poses(min_observations=6)
    pr = tctx.pose_refinements().tobytes()
    every_form(tctx, host, tracks, ids)
    assert tctx.pose_refinements().tobytes() == pr
    tctx.tracks_end()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_session_as_it_was(tctx, host):
    assert code(tctx.visibility) == _lib.E_STATE and code(tctx.visibility, basis="tracks") == _lib.E_STATE   # no track session
    ids, kps, poses, _, seen = efx.scene()
    d = np.random.default_rng(1).integers(0, 256, (efx.T, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(*pfx.match_list(seen, ids))
    assert code(tctx.visibility, basis="tracks") == _lib.E_STATE   # not finished
    tctx.tracks_finish()
    tracks = tctx.tracks()
    assert code(tctx.visibility) == _lib.E_STATE                   # basis MAP without points
    every_form(tctx, host, tracks, ids, "tracks")
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
    tctx.register_images(CAM, [int(ids[0])])
    before, reg = state(tctx), [a.tobytes() for a in tctx.registrations()]
    one = np.asarray([int(ids[0])], np.int32)
    qp = one.ctypes.data_as(C.POINTER(C.c_int32))

    def call(prm, q, n):
        return tctx._L.msfm_map_visibility(tctx._h, C.byref(_lib.VisibilityParams(*prm)), q, n, None, None, None)

    assert call((2, 0), None, 0) == _lib.E_INVALID and call((-1, 0), None, 0) == _lib.E_INVALID     # unknown basis
    assert call((1, 3), None, 0) == _lib.E_INVALID and call((0, -1), None, 0) == _lib.E_INVALID     # unknown route
    assert call((1, 0), qp, -1) == _lib.E_INVALID and call((1, 0), None, 1) == _lib.E_INVALID       # n_query < 0, NULL list
    assert code(tctx.visibility, [2]) == _lib.E_INVALID and code(tctx.visibility, [-5]) == _lib.E_INVALID   # not declared
    assert code(tctx.visibility, [int(ids[1]), int(ids[1])]) == _lib.E_INVALID                      # given twice
    assert b"given twice" in tctx._L.msfm_last_error(tctx._h)
    assert same_state(before, state(tctx)) and [a.tobytes() for a in tctx.registrations()] == reg
    # a streaming series open
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream([(int(ids[0]), int(ids[1])), (int(ids[1]), int(ids[2]))], max_distance=1e9)
    next(gen)
    assert code(tctx.visibility, basis="tracks") == _lib.E_STATE and code(tctx.visibility) == _lib.E_STATE
    gen.close()
    tctx.set_limits()
    every_form(tctx, host, tracks, ids)
    tctx.tracks_end()


def test_route_lds_is_refused_where_it_does_not_fit(tctx, host):
    """5462 declared images: their 3 x 5462 counter words exceed the 64 KiB of one workgroup (msfm_vis::vis_route reports no fit)."""
    n = 5462
    assert vtw.route(host, _lib.VIS_ROUTE_LDS, n, 0, 2, 4)["route"] == 0 and vtw.route(host, _lib.VIS_ROUTE_LDS, n - 1, 0, 2, 4)["route"] == 2
    ids = np.arange(n, dtype=np.int32)
    d = np.random.default_rng(1).integers(0, 256, (2, 128), dtype=np.uint8)
    for i in ids:
        tctx.upload_image(int(i), d)
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(np.asarray([[0, 1], [1, n - 1]], np.int32), np.asarray([0, 2, 3], np.int64), np.asarray([[0, 0], [1, 1], [0, 0]], np.int32))
    assert tctx.tracks_finish()["tracks_kept"] == 2
    tracks = tctx.tracks()
    assert code(tctx.visibility, (), "tracks", "lds") == _lib.E_INVALID
    want = vtw.run(host, tracks, ids, None, None, None, [n - 1, 0], "tracks")
    for name in ("global", "auto"):
        rec, mat, st = tctx.visibility([n - 1, 0], "tracks", name)
        assert rec.tobytes() == want[0].tobytes() and mat.tobytes() == want[1].tobytes() and st["route"] == _lib.VIS_ROUTE_GLOBAL
    assert mat[0, 1] == 1 and mat[1, 1] == 2 and mat[0, n - 1] == 1
    tctx.tracks_end()


# ---- the glue --------------------------------------------------------------------------------------------------------------------------
def two_view_records(poses, pairs, candidate=True):
    """records from the true relative poses: the pair's first image at (I, 0), its second at (R, t)"""
    out = {}
    for a, b in pairs:
        (Ra, ta), (Rb, tb) = poses[a], poses[b]
        r = np.zeros((), _lib.TWO_VIEW_RECORD)
        R = Rb @ Ra.T
        r["valid"], r["is_initial_candidate"], r["R"], r["t"] = 1, int(candidate), R.reshape(9), tb - R @ ta
        out[(a, b)] = r
    return out


def open_scene(ctx):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(ctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    return [int(i) for i in ids], kps, poses, seen


def test_initialize(tctx, host):
    ids, kps, poses, seen = open_scene(tctx)
    tracks = tctx.tracks()
    # the numpy reference's order of ALL pairs: first images by their elements, second images by what they share with the first
    rec, mat, _ = vref.run(tracks, ids, basis="tracks", query=ids)
    order = [(a, b) for a in _lib.initial_first_images(rec) for b in _lib.initial_second_images(mat[ids.index(a)], rec, a)]
    assert len(order) == len(ids) * (len(ids) - 1)
    picked = [order[7], order[3], order[12]]           # candidates; order[3] comes first
    two_view = two_view_records(poses, picked)
    two_view.update(two_view_records(poses, [order[1]], candidate=False))
    order0 = order[0]
    two_view[(order0[1], order0[0])] = np.zeros((), _lib.TWO_VIEW_RECORD)   # exists, not valid
    pair, trials, st = tctx.initialize(CAM, two_view, min_points=30, max_error=2.0, min_angle=1.0)
    assert pair == order[3] and trials == 1 and st["succeeded"] >= 30
    assert sorted(tctx.poses()) == sorted(pair) and np.array_equal(tctx.poses()[pair[0]][0], np.eye(3))
    # a record keyed the other way round is found, and its own first image stands at (I, 0)
    a, b = order[3]
    pair, trials, _ = tctx.initialize(CAM, two_view_records(poses, [(b, a)]), min_points=30, max_error=2.0, min_angle=1.0)
    assert pair == (b, a) and trials == 1 and np.array_equal(tctx.poses()[b][0], np.eye(3))
    # it stops at max_trials; every pair is a candidate, none reaches min_points
    every = two_view_records(poses, [p for p in order if p[0] < p[1]])
    pair, trials, st = tctx.initialize(CAM, every, max_trials=3, min_points=10 ** 6)
    assert pair is None and trials == 3 and st is not None
    pair, trials, st = tctx.initialize(CAM, two_view_records(poses, order[:5], candidate=False))
    assert (pair, trials, st) == (None, 0, None)
    tctx.tracks_end()


def test_grow_one_image_registers_the_best_seen(tctx, host):
    ids, kps, poses, seen = open_scene(tctx)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, np.asarray(ids), efx.FIRST), *THR)
    p0, _, m0, lst0 = state(tctx)
    first = _lib.next_images(vref.run(tracks, ids, lst0, p0, m0)[0])
    assert len(first) > 1
    reg, ext, alt, new = tctx.grow(CAM, max_images=1)
    assert new == [first[0]] and reg["images"] == 1 and ext["images_added"] == 1
    assert sorted(tctx.poses()) == sorted([ids[p] for p in efx.FIRST] + new)
    tctx.tracks_end()


def test_reconstruct_one_image_at_a_time_inside_a_window(tctx, host):
    """reconstruct(max_images=1, window=2): every image of the ring ends posed, one an increment; in every increment refine_poses
    holds every posed image outside {the new image, its two most covisible posed images} (by the numpy reference from the state at
    that moment), and only window poses carry REFINED in pose_refinements()."""
    ids, kps, poses, seen = open_scene(tctx)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, np.asarray(ids), efx.FIRST), *THR)
    real_points, real_poses, seen_states, seen_windows = tctx.refine_points, tctx.refine_poses, [], []

    def spy_points(**kw):   # (the state grow's visibility call saw: behind extend_points, before the alternation)
        p0, _, m0, lst0 = state(tctx)
        seen_states.append((lst0, p0, m0))
        return real_points(**kw)

    def spy_poses(fixed=(), **kw):
        st = real_poses(fixed=fixed, **kw)
        rec = tctx.pose_refinements()
        refined = {int(r["image_id"]) for r in rec if r["status"] & _lib.POSE_REFINED}
        seen_windows.append((sorted(vref.posed_ids(seen_states[-1][0])), sorted(int(i) for i in fixed), refined, seen_states[-1]))
        return st

    tctx.refine_points, tctx.refine_poses = spy_points, spy_poses
    out = tctx.reconstruct(CAM, rounds=1, max_images=1, window=2, pose_params=dict(min_observations=6))
    del tctx.refine_points, tctx.refine_poses
    assert sorted(tctx.poses()) == ids and len(out) == len(ids) - 3 and all(len(o["registered"]) == 1 for o in out)
    assert len(seen_windows) == len(out)
    for o, (posed, fixed, refined, (lst0, p0, m0)) in zip(out, seen_windows):
        new = o["registered"][0]
        rec, mat, _ = vref.run(tracks, ids, lst0, p0, m0, query=[new])
        window = {new} | set(_lib.local_window(mat[0], rec, new, size=2))
        assert len(window) == 3 and set(posed) - set(fixed) == window and refined <= window
    tctx.tracks_end()


class Spy:
    """the library with every call's name noted"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def test_grow_and_reconstruct_without_the_new_arguments(built_lib, host):
    """grow() / reconstruct() with max_images and window left at None: the same sequence of C calls and the same bytes as the direct
    sequence written out here -- the code path as it was before the two arguments existed."""
    logs, states = [], []
    for direct in (False, True):
        with _lib.Context(0) as ctx:
            ids, kps, poses, seen = open_scene(ctx)
            ctx.triangulate_tracks(CAM, some(poses, np.asarray(ids), efx.FIRST), *THR)
            log = []
            ctx._L = Spy(ctx._L, log)
            if not direct:
                ctx.grow(CAM, image_ids=[ids[4], ids[5]], rounds=1)
                out = ctx.reconstruct(CAM, rounds=1, max_increments=2)
                assert len(out) >= 1 and len(out[0]["registered"]) >= 1
            else:
                ctx.register_images(CAM, [ids[4], ids[5]])
                ctx.extend_points(_lib.registered_poses(ctx.registrations()[0]))
                ctx.refine_points()
                ctx.refine_poses()
                for _ in range(2):
                    posed = set(ctx.poses())
                    rest = [i for i in sorted(ids) if i not in posed]
                    if not rest:
                        break
                    ctx.register_images(CAM, rest)
                    new = _lib.registered_poses(ctx.registrations()[0])
                    if not new:
                        break
                    ctx.extend_points(new)
                    ctx.refine_points()
                    ctx.refine_poses()
                    ctx.filter_points()
            ctx._L = ctx._L._lib
            logs.append(log)
            states.append(state(ctx))
            ctx.tracks_end()
    assert logs[0] == logs[1] and "msfm_map_visibility" not in logs[0] and logs[0].count("msfm_register_images") >= 2
    assert same_state(states[0], states[1])
