"""Independent reference of the robust track triangulation (include/msfm_match.h "robust track triangulation"),
written from the definitions in plain numpy on top of tests/triangulation_ref.py: two-view and multi-view points from the STACKED rows
by numpy.linalg.svd (no normal equations, no Jacobi), errors in long double, angles by np.arccos, mix64 / sample2 on Python integers,
the best hypothesis by its own loop.  Test infrastructure only."""
import numpy as np

import triangulation_ref as ref

ROBUST = 32
LD = np.longdouble
M64 = (1 << 64) - 1
TRI_SEED = 0x547269616E67756C


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample2(seed, h, m):
    got = []
    for k in range(2):
        c, attempt = 0, 0
        while True:
            c = mix64(seed ^ mix64((h << 20) ^ (k << 8) ^ attempt)) % m if attempt < 32 else (c + 1) % m
            if c not in got:
                break
            attempt += 1
        got.append(int(c))
    return got


def hypotheses(m, max_hypotheses, track):
    """-> the list of (i, j), j < i, in hypothesis order"""
    every = [(i, j) for i in range(1, m) for j in range(i)]
    if len(every) <= max_hypotheses:
        return every
    seed = mix64(TRI_SEED ^ (int(track) & M64))
    return [(max(s), min(s)) for s in (sample2(seed, h, m) for h in range(max_hypotheses))]


def svd_point(obs):
    rows = []
    for u, v, P in obs:
        rows.append(float(u) * P[2] - P[0])
        rows.append(float(v) * P[2] - P[1])
    h = np.linalg.svd(np.asarray(rows, np.float64))[2][-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if h[3] == 0.0 or not np.all(np.isfinite(h[:3] / h[3])):
            return None
        return h[:3] / h[3]


def errors(X, obs, f):
    """-> (errors float [m], depth > eps bool [m]); the views at once, every sum in long double and in the order of the definition"""
    P = np.asarray([o[2] for o in obs], np.float64).astype(LD)
    u, v = np.asarray([o[0] for o in obs], LD), np.asarray([o[1] for o in obs], LD)
    Xl = np.asarray(X, np.float64).astype(LD)
    Y = P[:, :, 0] * Xl[0] + P[:, :, 1] * Xl[1] + P[:, :, 2] * Xl[2] + P[:, :, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (np.sqrt((Y[:, 0] / Y[:, 2] - u) ** 2 + (Y[:, 1] / Y[:, 2] - v) ** 2) * f).astype(np.float64)
    return e, Y[:, 2].astype(np.float64) > ref.EPS


TRACE_KEYS = ("retried", "m", "hypotheses", "winner", "best", "valid", "depth_rejected", "depth_rejected_best", "mask1", "mask2",
              "refit_stood", "flipped")


def track(img, idx, consistent, kps, poses, cam, track_no, max_error=2.0, min_angle=1.5, min_views=2, max_hypotheses=64, depth_check=True):
    """One track -> triangulation_ref.track's dict plus mask (element-aligned uint8), retried, hypotheses (H), literal_tie (the two
    best valid counts are equal), the margins taken over EVERY error and angle a decision of the definition looked at, and trace: the
    route the track took, from this function's own decisions (TRACE_KEYS, the fields of the twin's msfm_tri::RobustTrace).
    depth_check=False leaves the depth test out of a hypothesis' validity (NOT the definition: the tests use it to show that a track's
    answer hangs on that test)."""
    n = len(img)
    out = ref.track(img, idx, consistent, kps, poses, cam, max_error, min_angle, min_views)
    used = [k for k in range(n) if poses.get(int(img[k])) is not None]
    mask = np.zeros(n, np.uint8)
    if out["status"] & ref.ATTEMPTED:
        mask[used] = 1
    m = len(used) if out["status"] & ref.ATTEMPTED else 0
    tr = dict(retried=0, m=m, hypotheses=0, winner=-1, best=-1, valid=0, depth_rejected=0, depth_rejected_best=-1, mask1=-1, mask2=-1,
              refit_stood=0, flipped=0)
    out.update(mask=mask, retried=False, hypotheses=0, literal_tie=False, trace=tr)
    m = len(used)
    done = ref.POINT | ref.ERROR_OK
    if not out["status"] & ref.ATTEMPTED or (out["status"] & done) == done or m < 3:
        return out
    need = max(2, int(min_views))
    f = (LD(cam[0]) + LD(cam[1])) / 2
    obs = []
    for k in used:
        R, t = poses[int(img[k])]
        P = np.c_[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)]
        u, v = ref.observation(cam, kps[int(img[k])][int(idx[k]), :2])
        obs.append((u, v, P))
    centres = [-(P[:, :3].astype(LD).T @ P[:, 3].astype(LD)) for _, _, P in obs]
    em, am = [out["error_margin"]], [out["angle_margin"]]
    hyp = hypotheses(m, max_hypotheses, track_no)
    best, best_X, counts = -1, None, []
    for h, (i, j) in enumerate(hyp):
        X = svd_point([obs[j], obs[i]])
        if X is None:
            continue
        e, d = errors(X, obs, f)
        a = ref.angle(X, centres[i], centres[j])
        em.append(float(np.min(np.abs(e - max_error))))
        am.append(abs(a - min_angle))
        c = int(np.sum(d & (e <= max_error)))
        if a >= min_angle and not (d[i] and d[j]):
            tr["depth_rejected"] += 1
            tr["depth_rejected_best"] = max(tr["depth_rejected_best"], c)
        if not (((d[i] and d[j]) or not depth_check) and a >= min_angle):
            continue
        tr["valid"] += 1
        counts.append(c)
        if c > best:
            best, best_X = c, X
            tr["winner"] = h
    counts.sort()
    tr.update(retried=1, hypotheses=len(hyp), best=best)
    out.update(retried=True, hypotheses=len(hyp), literal_tie=len(counts) >= 2 and counts[-1] == counts[-2])
    out.update(status=ref.ATTEMPTED | ROBUST, n_views=0, X=np.zeros(3), mean_residual=0.0, tri_angle=0.0, residuals=np.full(n, -1.0),
               mask=np.zeros(n, np.uint8), error_margin=min(em), angle_margin=min(am))
    if best < need:
        return out
    e, d = errors(best_X, obs, f)
    m1 = d & (e <= max_error)
    X = best_X
    inl = m1
    tr["mask1"] = int(m1.sum())
    X1 = svd_point([o for o, keep in zip(obs, m1) if keep])
    if X1 is not None:
        e1, d1 = errors(X1, obs, f)
        em.append(float(np.min(np.abs(e1 - max_error))))
        m2 = d1 & (e1 <= max_error)
        tr["mask2"] = int(m2.sum())
        if m2.sum() >= max(m1.sum(), need):
            X, inl = X1, m2
            tr["refit_stood"] = 1
    tr["flipped"] = int(np.sum(m1 != inl))
    e, d = errors(X, obs, f)
    status = ref.ATTEMPTED | ref.POINT | ref.ERROR_OK | ROBUST | (ref.DEPTH_OK if np.all(d[inl]) else 0)
    res = np.full(n, -1.0)
    res[used] = e
    mask = np.zeros(n, np.uint8)
    mask[np.asarray(used)[inl]] = 1
    pos = [p for p in range(m) if inl[p]]
    angle, hit = 0.0, False
    for a_ in range(len(pos)):
        for b_ in range(a_):
            g = ref.angle(X, centres[pos[a_]], centres[pos[b_]])
            am.append(abs(g - min_angle))
            if g >= min_angle:
                angle, hit = g, True
                break
            angle = max(angle, g)
        if hit:
            break
    out.update(status=status | (ref.ANGLE_OK if hit else 0), n_views=int(inl.sum()), X=X, tri_angle=angle, residuals=res, mask=mask,
               mean_residual=float(np.sum(np.asarray(e[inl], LD)) / int(inl.sum())), error_margin=min(em), angle_margin=min(am))
    return out


def run(tracks, kps, poses, cam, max_error=2.0, min_angle=1.5, min_views=2, max_hypotheses=64, select=None, depth_check=True):
    offsets, img, idx, cons = tracks[:4]
    todo = range(len(offsets) - 1) if select is None else select
    return [track(img[offsets[t]:offsets[t + 1]], idx[offsets[t]:offsets[t + 1]], bool(cons[t]), kps, poses, cam, t, max_error, min_angle,
                  min_views, max_hypotheses, depth_check) for t in todo]
