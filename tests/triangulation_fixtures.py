"""Inputs and checks shared by the plain track triangulation's CPU and GPU edge tests (tests/test_triangulation_fixtures.py drives them
with the host twin, tests/test_gpu_triangulation_edges.py with the device): a hand-built job with every exit of triangulate_track
planted at the wave and block edges, the thresholds met with equality, the parameters at their limits, the scan order, and the
ill-conditioned scenes of tests/test_triangulation_reference.py as track sessions.  Every check takes a callable
run(params=tw.DEFAULTS, poses=None, cam=CAM) -> (points, residuals) over one job, so it is written once.  Test infrastructure only."""
import functools

import numpy as np

import triangulation_ref as ref
import triangulation_twin as tw

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)
N_TRACKS = 257
EDGES = (0, 63, 64, 255, 256)          # first lane, last lane of wave 0, first of wave 1, last lane of block 0, the lone lane of block 1
PREFIXES = (256, 255, 65, 64, 63, 1)
RING = 32                              # ring positions 0 .. 30 are ring_job's cameras, 1.2 degrees apart; position 31 is turned round
TURNED = RING - 1
SUCCEEDED = 31
# the exits of triangulate_track and the status word each leaves under the defaults (2 px, 1.5 degrees, 2 views)
ROUTE_STATUS = dict(few_views=0, inconsistent=0, no_point=1, error=27, angle=23, depth=15)
ROUTES = tuple(ROUTE_STATUS)
NO_RESIDUALS = ("few_views", "inconsistent", "no_point")   # every residual slot of the track is -1
V, I, N, E, A, D = ROUTES
# position -> route.  Layout 0 is the one the prefixes run: both neighbours of every track without residuals SUCCEED there, so the
# four edge lanes that touch each other (63 | 64, 255 | 256) hold exits with a point.  Layouts 1 .. 6 turn the routes round until
# every route has stood at every edge lane; there a neighbour of a track without residuals may be one of the exits with a point
# (whose posed slots are not -1 either).
LAYOUTS = (
    {0: N, 61: I, 63: E, 64: D, 66: V, 253: N, 255: A, 256: E},
    {0: I, 2: D, 63: V, 64: E, 255: N, 256: A},
    {0: V, 2: A, 63: D, 64: I, 255: E, 256: N},
    {0: E, 2: I, 63: N, 64: A, 255: D, 256: V},
    {0: A, 2: N, 4: E, 63: A, 64: V, 255: I, 256: D},
    {0: D, 2: N, 4: A, 63: I, 64: E, 255: V, 256: E},
    {0: E, 2: V, 63: D, 64: N, 255: A, 256: I},
)


@functools.lru_cache(maxsize=None)
def ring():
    """ring_job's cameras with N_TRACKS scene points seen by all of them (0.3 px of noise): the pool the tracks draw their elements
    from -> (kps per ring position, pose per ring position)"""
    # (ring_job, laid_out, open_ring and second_pass_job live in a GPU test module, which does nothing on import)
    from test_gpu_robust_triangulation import ring_job
    ids, kps, poses, _ = ring_job([RING] * N_TRACKS, noise_px=0.3, seed=21, turned=(TURNED,))
    return kps, [poses[int(i)] for i in ids]


def tracks_of(laid, joined=()):
    """the track result of laid_out(laid): track j through its own images at keypoint row 0; a track in `joined` also holds row 1 of
    its first image (two keypoints of one image: inconsistent)"""
    offs, img, idx, cons, at = [0], [], [], [], 0
    for j, (ps, _) in enumerate(laid):
        el = [(3 * (at + k) + 1, 0) for k in range(len(ps))]
        if j in joined:
            el.insert(1, (el[0][0], 1))
        img += [e[0] for e in el]
        idx += [e[1] for e in el]
        offs.append(offs[-1] + len(el))
        cons.append(0 if j in joined else 1)
        at += len(ps)
    return np.asarray(offs, np.int64), np.asarray(img, np.int32), np.asarray(idx, np.int32), np.asarray(cons, np.uint8)


def laid_job(laid, joined=()):
    """laid_out(laid) as a job dict(ids, kps, poses, lst, tracks); for a track in `joined` one more match, (its first image's row 1,
    its second image's row 0), joins a second keypoint of the first image to the track"""
    from test_gpu_robust_triangulation import laid_out
    ids, kps, poses, lst = laid_out(laid)
    at = np.concatenate([[0], np.cumsum([len(p) for p, _ in laid])])
    for j in joined:
        a, b = ids[at[j]], ids[at[j] + 1]
        lst = (np.r_[lst[0], [[a, b]]].astype(np.int32), np.r_[lst[1], lst[1][-1] + 1], np.r_[lst[2], [[1, 0]]].astype(np.int32))
    return dict(ids=ids, kps=kps, poses=poses, lst=lst, tracks=tracks_of(laid, joined), joined=tuple(joined))


def open_job(ctx, job):
    """the job as a finished track session on the device, inconsistent tracks kept; the device's track result is the job's"""
    from test_gpu_robust_triangulation import open_ring
    open_ring(ctx, job["ids"], job["kps"], job["lst"], 2)
    ts = ctx.tracks_finish(keep_inconsistent=True)
    got = ctx.tracks()
    assert ts["tracks_kept"] == len(job["tracks"][0]) - 1 and all(a.tobytes() == b.tobytes() for a, b in zip(got, job["tracks"]))
    return got


def routes_job(T=N_TRACKS, layout=0):
    """The first T of 257 tracks of 2 .. 5 elements, every element in an image of its own (laid_out).  The tracks at the positions of
    LAYOUTS[layout] take one exit of triangulate_track each, all others succeed (two to five ring cameras at even positions, at least
    2.4 degrees apart; every fifth with an unposed element in the middle):
        few_views     three elements, one posed
        inconsistent  two views and a second keypoint of the first image
        no_point      two views, the second with t = (1e200, 0, 6.5)
        error         four views, one observation moved by 40 px
        angle         two views at neighbouring ring positions, 1.2 degrees apart
        depth         three views, the last through the camera that is turned round
    A prefix (T < 257) is the same job cut behind track T - 1: the same images, keypoints and poses.
    -> dict(ids, kps, poses, lst, tracks, joined, planted = {position: route} below T)"""
    kps, pose = ring()
    rng = np.random.default_rng(33)
    plan = LAYOUTS[layout]
    laid, joined = [], []
    for j in range(N_TRACKS):
        even = rng.permutation(np.arange(0, TURNED, 2))
        route = plan.get(j)
        n = 2 + j % 4
        pos = [int(p) for p in even[:n]]
        if route in (I, N):
            pos = pos[:2]
        elif route == V:
            pos = [int(p) for p in even[:3]]
        elif route == E:
            pos = [int(p) for p in even[:4]]
        elif route == A:
            pos = [pos[0], pos[0] + 1 if pos[0] + 1 < TURNED else pos[0] - 1]
        elif route == D:
            pos = [int(p) for p in even[:2]] + [TURNED]
        ps = [pose[p] for p in pos]
        xy = np.asarray([kps[p][j, :2] for p in pos], np.float32)
        if route == V:
            ps[1] = ps[2] = None
        elif route == N:
            ps[1] = (ps[1][0], np.asarray([1e200, 0.0, 6.5]))
        elif route == E:
            xy[1, 0] += np.float32(40.0)
        elif route == I:
            joined.append(j)
        elif route is None and j % 5 == 3 and n < 5:
            ps.insert(1, None)
            xy = np.insert(xy, 1, xy[0], axis=0)
        laid.append((ps, xy))
    job = laid_job(laid[:T], [j for j in joined if j < T])
    job["planted"] = {p: r for p, r in plan.items() if p < T}
    return job


def twin_run(host, job):
    """the callable the checks take, on the host twin"""
    def run(params=tw.DEFAULTS, poses=None, cam=CAM):
        return tw.run(host, job["tracks"], job["ids"], job["kps"], job["poses"] if poses is None else poses, cam, params)
    return run


def routes(host, job, cam=CAM):
    """The twin under the defaults -> (points, residuals, {route: track numbers}) with "succeeded" among the routes, found from the
    status words (and the session's flag, which tells the two exits that leave 0 apart).  Raises if a track planted below T did not
    take its route, or another track took one."""
    pts, res = twin_run(host, job)(cam=cam)
    s, cons = pts["status"], job["tracks"][3]
    found = {r: np.nonzero((s == w) & (cons == (0 if r == I else 1)))[0].tolist() for r, w in ROUTE_STATUS.items()}
    found["succeeded"] = np.nonzero(s == SUCCEEDED)[0].tolist()
    want = {r: sorted(p for p, q in job["planted"].items() if q == r) for r in ROUTES}
    if any(found[r] != want[r] for r in ROUTES) or sum(len(v) for v in found.values()) != len(s):
        raise ValueError("planted %s, found %s, status words %s" % (want, found, sorted(set(s.tolist()))))
    return pts, res, found


def used_elements(job, t, poses=None):
    """the elements of track t whose image is posed -> their positions in the track"""
    o, img = job["tracks"][0], job["tracks"][1]
    poses = job["poses"] if poses is None else poses
    return [k for k in range(int(o[t + 1] - o[t])) if poses.get(int(img[o[t] + k])) is not None]


def neighbours_hold_residuals(job, pts, res):
    """both neighbours of every track without residuals have a point, and no -1 in the slot of a posed element: a write outside a
    track's own slots would land on a value that is not -1.  -> the tracks without residuals"""
    o = job["tracks"][0]
    bare = [t for t in range(len(pts)) if not int(pts[t]["status"]) & ref.POINT]
    for t in bare:
        assert np.all(res[o[t]:o[t + 1]] == -1.0), t
        for nb in (t - 1, t + 1):
            if 0 <= nb < len(pts):
                assert int(pts[nb]["status"]) & ref.POINT, (t, nb)
                assert np.all(res[o[nb]:o[nb + 1]][used_elements(job, nb)] >= 0.0), (t, nb)
    return bare


def verdicts_follow(job, pts, res, params, poses=None):
    """what the record's own numbers fix of its status word, under any parameters: ATTEMPTED and n_views from the posed elements,
    ERROR_OK iff every used residual <= max_error, ANGLE_OK iff tri_angle >= min_angle, -1 exactly in the unused slots"""
    o, cons = job["tracks"][0], job["tracks"][3]
    need = max(2, int(params[2]))
    for t in range(len(pts)):
        used, s, r = used_elements(job, t, poses), int(pts[t]["status"]), res[o[t]:o[t + 1]]
        if not cons[t] or len(used) < need:
            assert pts[t].tobytes() == bytes(48) and np.all(r == -1.0), t
            continue
        assert s & ref.ATTEMPTED and int(pts[t]["n_views"]) == len(used), t
        if not s & ref.POINT:
            assert s == ref.ATTEMPTED and pts[t].tobytes()[8:] == bytes(40) and np.all(r == -1.0), t
            continue
        assert np.array_equal(np.nonzero(r >= 0.0)[0], used) and np.all(r[r < 0.0] == -1.0), t
        assert bool(s & ref.ERROR_OK) == bool(np.all(r[used] <= params[0])), t
        assert bool(s & ref.ANGLE_OK) == bool(float(pts[t]["tri_angle"]) >= params[1]), t


def equality_tracks(job, pts):
    """-> (three tracks with a point for the error threshold: lanes 63 and 64 and one interior; three two-view tracks with a point for
    the angle: the last of wave 0, the first of wave 1, the last of all)"""
    o, s = job["tracks"][0], pts["status"]
    interior = next(t for t in range(100, len(pts)) if s[t] == SUCCEEDED and o[t + 1] - o[t] >= 3)
    two = [t for t in range(len(pts)) if s[t] & ref.POINT and len(used_elements(job, t)) == 2]
    return (63, 64, interior), (max(t for t in two if t < 64), min(t for t in two if t >= 64), max(two))


def equality_checks(run, job):
    """err <= max_error and angle >= min_angle met with equality.  The thresholds are the caller's own numbers: the largest residual
    of a track and the tri_angle of a two-view track as `run` itself reports them, then one place below / above.
    -> {track: (e or a, status at equality, status one place off)} for the record"""
    o = job["tracks"][0]
    p0, r0 = run()
    err_tracks, ang_tracks = equality_tracks(job, p0)
    seen = {}
    for t in err_tracks:
        assert int(p0[t]["status"]) & ref.POINT
        e = float(r0[o[t]:o[t + 1]].max())
        assert e > 0.0 and np.isfinite(e)
        p1, r1 = run((e, 1.5, 2))
        assert int(p1[t]["status"]) & ref.ERROR_OK, (t, e)
        below = float(np.nextafter(e, 0.0))
        p2, r2 = run((below, 1.5, 2))
        assert not int(p2[t]["status"]) & ref.ERROR_OK, (t, e)
        for p, r, prm in ((p1, r1, (e, 1.5, 2)), (p2, r2, (below, 1.5, 2))):
            assert r.tobytes() == r0.tobytes() and p["X"].tobytes() == p0["X"].tobytes()
            assert all(p[f].tobytes() == p0[f].tobytes() for f in ("n_views", "mean_residual", "tri_angle"))
            verdicts_follow(job, p, r, prm)
        seen[t] = (e, int(p1[t]["status"]), int(p2[t]["status"]))
    pa, ra = run((2.0, 0.0, 2))
    for t in ang_tracks:
        assert int(pa[t]["status"]) & ref.ANGLE_OK
        a = float(pa[t]["tri_angle"])
        assert 0.0 < a < 90.0
        p1, r1 = run((2.0, a, 2))
        assert int(p1[t]["status"]) & ref.ANGLE_OK and float(p1[t]["tri_angle"]) == a, (t, a)
        above = float(np.nextafter(a, 100.0))
        p2, r2 = run((2.0, above, 2))
        assert not int(p2[t]["status"]) & ref.ANGLE_OK and float(p2[t]["tri_angle"]) == a, (t, a)
        for p, r, prm in ((p1, r1, (2.0, a, 2)), (p2, r2, (2.0, above, 2))):
            assert r.tobytes() == ra.tobytes() and p["X"].tobytes() == pa["X"].tobytes()
            verdicts_follow(job, p, r, prm)
        seen[t] = (a, int(p1[t]["status"]), int(p2[t]["status"]))
    return seen


def pair_angles(job, t, X):
    """the reference's parallax angle at X of every pair of used observations of track t, in scan order (for i: for j < i)
    -> [((i, j), degrees)] with i, j the elements' positions in the track"""
    o, img = job["tracks"][0], job["tracks"][1]
    used = used_elements(job, t)
    cen = {}
    for k in used:
        R, tt = job["poses"][int(img[o[t] + k])]
        cen[k] = -(np.asarray(R, ref.LD).T @ np.asarray(tt, ref.LD))
    return [((i, j), ref.angle(X, cen[i], cen[j])) for n, i in enumerate(used) for j in used[:n]]


MIN_VIEWS = (-5, 0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1)   # (3 .. 6: the length and the length + 1 of every track of 2 .. 5 elements)


def parameter_checks(run, job, tol_angle):
    """min_views, max_error and min_angle at their limits; tol_angle: the bound of |tri_angle - the reference's angle|"""
    o = job["tracks"][0]
    p0, r0 = run()
    T = len(p0)
    assert T > 0 and (p0["status"] & ref.POINT).any()
    lengths = {len(used_elements(job, t)) for t in range(T)}
    assert lengths >= {1, 2, 3, 4, 5}
    for mv in MIN_VIEWS:
        p, r = run((2.0, 1.5, mv))
        verdicts_follow(job, p, r, (2.0, 1.5, mv))
        if mv <= 2:
            assert p.tobytes() == p0.tobytes() and r.tobytes() == r0.tobytes(), mv
        elif mv == 2 ** 31 - 1:
            assert p.tobytes() == bytes(48 * T) and np.all(r == -1.0)
        else:   # a track is attempted or not; what it computes does not depend on min_views
            kept = np.asarray([len(used_elements(job, t)) >= mv for t in range(T)]) & (p0["status"] != 0)
            assert kept.any() == (mv <= 5) and not kept.all()
            assert p[kept].tobytes() == p0[kept].tobytes() and p[~kept].tobytes() == bytes(48 * int((~kept).sum())), mv
            per_obs = np.repeat(kept, np.diff(o))
            assert r[per_obs].tobytes() == r0[per_obs].tobytes() and np.all(r[~per_obs] == -1.0), mv
    with_point = (p0["status"] & ref.POINT) != 0
    for me in (0.0, 1e300):
        p, r = run((me, 1.5, 2))
        verdicts_follow(job, p, r, (me, 1.5, 2))
        assert r.tobytes() == r0.tobytes() and p["X"].tobytes() == p0["X"].tobytes()
        assert np.array_equal((p["status"] & ref.POINT) != 0, with_point)
        assert np.all(((p["status"] & ref.ERROR_OK) != 0) == (with_point if me else np.zeros(T, bool))), me
    worst = 0.0
    for ma in (0.0, 90.0, 91.0):
        p, r = run((2.0, ma, 2))
        verdicts_follow(job, p, r, (2.0, ma, 2))
        assert r.tobytes() == r0.tobytes() and p["X"].tobytes() == p0["X"].tobytes()
        if ma == 90.0:   # (no claim about which tracks reach 90 degrees: the record's own angle decides, verdicts_follow)
            continue
        assert np.all(((p["status"] & ref.ANGLE_OK) != 0) == (with_point if ma == 0.0 else np.zeros(T, bool))), ma
        for t in np.nonzero(with_point)[0]:
            angles = [a for _, a in pair_angles(job, t, p[t]["X"])]
            want = angles[0] if ma == 0.0 else max(angles)
            worst = max(worst, abs(float(p[t]["tri_angle"]) - want))
            assert abs(float(p[t]["tri_angle"]) - want) <= tol_angle, (ma, t, float(p[t]["tri_angle"]), want)
    return worst


SCAN_USED = (1, 3, 4, 5)
SCAN_POSITIONS = {1: 10, 3: 9, 4: 12, 5: 16}


def scan_order_job():
    """One track of six elements, elements 0 and 2 unposed; the used ones stand at the ring positions 10, 9, 12 and 16.  The scan meets
    (3, 1) first, then (4, 1), where it must stop; walked the other way (j downwards) it would meet (4, 3) before (4, 1), and the
    largest-angle rule would give (5, 3).  The reference's angles at the twin's point, computed on the CPU:
        (3, 1) 1.2840 degrees   below min_angle = 1.5
        (4, 1) 2.5749 degrees   the first pair that reaches it: tri_angle
        (4, 3) 3.8590 degrees   reaches it too, later in scan order
        (5, 1) 7.7513 degrees   larger still, never scanned
    -> the job"""
    kps, pose = ring()
    ps = [None] * 6
    for k, p in SCAN_POSITIONS.items():
        ps[k] = pose[p]
    xy = np.asarray([kps[SCAN_POSITIONS.get(k, 0)][0, :2] for k in range(6)], np.float32)
    return laid_job([(ps, xy)])


def scan_order_check(run, job, tol_angle, min_angle=1.5):
    """tri_angle is the angle of (4, 1).  On the reference alone first: the three angles of the docstring lie on their sides of
    min_angle, each at least 0.1 degrees away from it.  -> {(i, j): reference angle}"""
    pts, _ = run((2.0, min_angle, 2))
    assert int(pts[0]["status"]) == SUCCEEDED and int(pts[0]["n_views"]) == 4
    ang = dict(pair_angles(job, 0, pts[0]["X"]))
    assert list(ang)[:2] == [(3, 1), (4, 1)]
    assert ang[(3, 1)] <= min_angle - 0.1 and min_angle + 0.1 <= ang[(4, 1)] <= ang[(5, 1)] - 0.1 and ang[(4, 3)] >= ang[(4, 1)] + 0.1
    assert abs(float(pts[0]["tri_angle"]) - ang[(4, 1)]) <= tol_angle, (float(pts[0]["tri_angle"]), ang)
    return ang


def capture_list(tracks):
    """a track result as a list for tracks_add: the consecutive elements of every track joined pair by pair"""
    o, img, idx, _ = tracks
    first = np.ones(len(img), bool)
    first[o[:-1]] = False
    b = np.nonzero(first)[0]                                    # element b is joined to element b - 1
    key = img[b - 1].astype(np.int64) * (1 << 32) + img[b]
    order = np.argsort(key, kind="stable")
    uniq, start = np.unique(key[order], return_index=True)
    pairs = np.stack([uniq >> 32, uniq & 0xFFFFFFFF], 1).astype(np.int32)
    offs = np.r_[start, len(order)].astype(np.int64)
    qt = np.stack([idx[b - 1][order], idx[b][order]], 1).astype(np.int32)
    return pairs, offs, qt


# The 20 tracks of the seed-5 capture (0.3 px) whose twin point lies farthest from the 50-digit solution, per case of
# test_triangulation_reference.MP_CASES, farthest first; computed on the CPU by that module's mp_case and checked against it in
# tests/test_triangulation_fixtures.py.  The device test bounds these by MP_BOUNDS without solving all 1439 tracks in mpmath.
MP_WORST = {
    "shift 1e2": [1368, 534, 1284, 1277, 841, 999, 1428, 863, 1186, 313, 893, 247, 1013, 459, 805, 1157, 1033, 1378, 91, 1053],        # 4.7e-11 .. 1.3e-12
    "shift 1e4": [1368, 1186, 1013, 841, 863, 1284, 1401, 1350, 877, 1277, 1066, 1276, 1321, 1402, 1428, 806, 25, 805, 1162, 770],     # 7.5e-9 .. 1.0e-10
    "shift 1e6": [1368, 1186, 1284, 1428, 1277, 689, 1138, 1276, 1321, 1013, 770, 1430, 1042, 1057, 345, 863, 384, 1039, 1353, 1009],  # 2.8e-7 .. 1.2e-8
    "scale 1e-3": [1186, 1368, 1284, 863, 689, 1428, 313, 1431, 1350, 726, 1321, 1366, 474, 534, 336, 1009, 247, 1401, 811, 1042],     # 1.4e-16 .. 7.8e-18
    "scale 1e6": [1186, 1368, 1431, 1428, 1284, 1366, 841, 1430, 863, 247, 1401, 1063, 1051, 1333, 534, 741, 1066, 726, 576, 689],     # 3.4e-7 .. 1.5e-8
}


def conditioning_jobs():
    """-> (capture: the seed-5 capture of test_triangulation_reference with `lst`, its tracks as a tracks_add list, and `cases` =
    [(name, poses)] under each of MP_CASES;  small: small_parallax_tracks() as a laid_out job, to run under min_angle = 0)"""
    import test_triangulation_reference as tb
    c = tb.capture(5, noise_px=0.3)
    c["lst"] = capture_list(c["tracks"])
    c["cases"] = [(name, fn(c["poses"], mag)) for name, fn, mag in tb.MP_CASES]
    return c, laid_job(tb.small_parallax_tracks()[0])


def mp_distance(c, poses, pts, t):
    """|X - X_mp| of track t of the capture under `poses`: the record's point against mp_point of the same stacked rows"""
    o, img, idx, _ = c["tracks"]
    obs = [ref.observation(c["cam"], c["kps"][int(img[e])][int(idx[e]), :2]) + (np.c_[poses[int(img[e])][0], poses[int(img[e])][1]],)
           for e in range(int(o[t]), int(o[t + 1]))]
    return float(np.abs(pts[t]["X"] - ref.mp_points([obs])[0]).max())
