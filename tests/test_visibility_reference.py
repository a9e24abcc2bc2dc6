"""The map visibility's host twin (csrc/msfm_visibility.h, MapVisibility) against an independent numpy reference
(tests/visibility_ref.py), array for array and counter for counter -- integer counting, so the comparison is exact -- and the
invariants the definitions of include/msfm_match.h "map visibility" imply, on every case.  No GPU."""
import numpy as np
import pytest

import filter_fixtures as ffx
import visibility_ref as vref
import visibility_twin as vtw
from monocularsfm_amd import _lib

OK = vref.OK


@pytest.fixture(scope="module")
def host():
    return vtw.load_host()


def check(host, tracks, ids, pose_list, points, mask, query, basis):
    """twin == reference, and the invariants; -> the twin's result"""
    got = vtw.run(host, tracks, ids, pose_list, points, mask, query, basis)
    want = vref.run(tracks, ids, pose_list, points, mask, query, basis)
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes()
    assert got[2] == want[2]
    rec, mat, cnt = got
    order = sorted(int(i) for i in ids)
    at = {i: k for k, i in enumerate(order)}
    posed = (rec["flags"] & _lib.VIS_POSED) != 0
    assert cnt["pair_increments"] == int(mat.sum(dtype=np.int64))
    if basis == "tracks":
        assert np.array_equal(rec["n_visible"], rec["n_elements"]) and not rec["n_points"].any() and not posed.any()
    assert np.all(rec["n_visible"] <= rec["n_elements"]) and np.all(rec["n_points"] <= rec["n_visible"])
    assert np.all(rec["n_points"][~posed] == 0)
    # the diagonal entry: the image's counting elements (n_points where it is posed, n_visible where it is not)
    for r, i in enumerate(query):
        own = int(mat[r, at[int(i)]])
        assert own == int(rec["n_points"][at[int(i)]] if posed[at[int(i)]] else rec["n_visible"][at[int(i)]])
        assert np.all(mat[r] <= own)
    assert cnt["elements_counted"] == int(np.where(posed, rec["n_points"], rec["n_visible"]).sum())
    return got


def full(host, tracks, ids, pose_list, points, mask, basis):
    """query = every image: the matrix is symmetric; an image's row against an image it shares no standing track with is 0"""
    order = sorted(int(i) for i in ids)
    rec, mat, cnt = check(host, tracks, ids, pose_list, points, mask, order, basis)
    assert np.array_equal(mat, mat.T)
    offsets, img, cons = np.asarray(tracks[0]), np.asarray(tracks[1]), np.asarray(tracks[3])
    T = len(offsets) - 1
    standing = cons != 0 if basis == "tracks" else (cons != 0) & ((points["status"][:T] & OK) == OK)
    share = np.zeros((len(order), len(order)), bool)
    for t in np.flatnonzero(standing):
        c = np.searchsorted(order, img[offsets[t]:offsets[t + 1]])
        share[np.ix_(c, c)] = True
    assert not mat[~share].any()
    return rec, mat, cnt


@pytest.mark.parametrize("name", sorted(ffx.CASES))
def test_ring_fixtures(host, name):
    s = ffx.CASES[name](host)
    pp, _, pm = s["before"]
    ids = [int(i) for i in s["ids"]]
    for basis in ("map", "tracks"):
        full(host, s["tracks"], ids, s["lst"], pp, pm, basis)
        check(host, s["tracks"], ids, s["lst"], pp, pm, (), basis)
        check(host, s["tracks"], ids, s["lst"], pp, pm, ids[3:0:-1], basis)
    rec = check(host, s["tracks"], ids, s["lst"], pp, pm, (), "map")[0]
    assert rec["n_points"].sum() > 0
    if pm is not None and not pm.all():   # rejected observations of standing points: seen, not counted
        assert (rec["n_points"] < rec["n_visible"])[(rec["flags"] & _lib.VIS_POSED) != 0].any()


def random_session(seed, n=9, T=300, with_mask=True, posed_frac=0.5):
    """random consistent and inconsistent tracks over n images with gaps in their ids, random status bits, a random posed set"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(3, 60), n, replace=False)).astype(np.int32)
    offsets, img, cons = [0], [], []
    for _ in range(T):
        ln = int(rng.integers(2, n + 1))
        consistent = rng.random() < 0.8
        if consistent:
            el = np.sort(rng.choice(ids, ln, replace=False))
        else:
            el = np.sort(rng.choice(ids, ln + 1, replace=True))   # (an image twice, mostly)
        img.extend(int(i) for i in el)
        offsets.append(len(img))
        cons.append(1 if consistent else 0)
    tracks = (np.asarray(offsets, np.int64), np.asarray(img, np.int32), np.zeros(len(img), np.int32), np.asarray(cons, np.uint8))
    points = np.zeros(T, _lib.POINT3D)
    points["status"] = rng.choice([0, 1, 3, 7, 11, 15, 31, 15 | 512, 1 | 512, 15 | 1024, 3 | 64], T)
    listed = [int(i) for i in ids if rng.random() < 0.8]
    poses = {i: ((np.eye(3), np.zeros(3)) if rng.random() < posed_frac / 0.8 else None) for i in listed}
    mask = (rng.random(len(img)) < 0.7).astype(np.uint8) if with_mask else None
    return tracks, [int(i) for i in ids], poses, points, mask


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("with_mask", [False, True])
def test_random_sessions(host, seed, with_mask):
    tracks, ids, poses, points, mask = random_session(seed, with_mask=with_mask)
    rng = np.random.default_rng(100 + seed)
    for basis in ("map", "tracks"):
        rec, mat, cnt = full(host, tracks, ids, poses, points, mask, basis)
        assert cnt["tracks_counted"] > 0 and mat.any()
        q = [int(i) for i in rng.permutation(ids)[:4]]
        check(host, tracks, ids, poses, points, mask, q, basis)
        check(host, tracks, ids, poses, points, mask, (), basis)
    # the inconsistent tracks change no counter
    keep = np.flatnonzero(tracks[3])
    offs = np.concatenate([[0], np.cumsum(np.diff(tracks[0])[keep])])
    sel = np.concatenate([np.arange(tracks[0][t], tracks[0][t + 1]) for t in keep])
    only = (offs, tracks[1][sel], tracks[2][sel], tracks[3][keep])
    a = vtw.run(host, tracks, ids, poses, points, mask, ids, "map")
    b = vtw.run(host, only, ids, poses, points[keep], None if mask is None else mask[sel], ids, "map")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_listed_image_with_an_invalid_pose(host):
    tracks, ids, poses, points, mask = random_session(7)
    unposed = [i for i, p in poses.items() if p is None]
    assert unposed
    rec, mat, _ = full(host, tracks, ids, poses, points, mask, "map")
    at = {int(r["image_id"]): k for k, r in enumerate(rec)}
    for i in unposed:   # listed without a pose = not listed: every element of a standing track counts
        assert not rec["flags"][at[i]] & _lib.VIS_POSED and rec["n_points"][at[i]] == 0
        assert mat[at[i], at[i]] == rec["n_visible"][at[i]]
    dropped = {i: p for i, p in poses.items() if p is not None}
    again = vtw.run(host, tracks, ids, dropped, points, mask, ids, "map")
    assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == mat.tobytes()


def test_removed_point(host):
    """ATTEMPTED | FILTERED and nothing else: the point does not stand; its elements are elements, not visible"""
    tracks, ids, poses, points, mask = random_session(9, T=40)
    points["status"] = 15
    before = full(host, tracks, ids, poses, points, mask, "map")
    t = int(np.flatnonzero(tracks[3])[0])
    points["status"][t] = _lib.TRI_ATTEMPTED | _lib.TRI_FILTERED
    after = full(host, tracks, ids, poses, points, mask, "map")
    assert after[2]["tracks_counted"] == before[2]["tracks_counted"] - 1
    assert np.array_equal(after[0]["n_elements"], before[0]["n_elements"])
    assert before[0]["n_visible"].sum() - after[0]["n_visible"].sum() == tracks[0][t + 1] - tracks[0][t]


def test_no_tracks(host):
    tracks = (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    ids = [4, 9, 11]
    for basis in ("map", "tracks"):
        rec, mat, cnt = full(host, tracks, ids, {4: (np.eye(3), np.zeros(3))}, np.zeros(0, _lib.POINT3D), None, basis)
        assert not mat.any() and cnt == dict.fromkeys(vtw.COUNT_KEYS, 0)
        assert list(rec["image_id"]) == ids and not rec["n_elements"].any()


@pytest.mark.parametrize("with_mask", [False, True])
def test_every_image_unposed(host, with_mask):
    tracks, ids, _, points, mask = random_session(11, with_mask=with_mask)
    for poses in (None, {}, {i: None for i in ids}):
        rec, mat, cnt = full(host, tracks, ids, poses, points, mask, "map")
        assert not rec["flags"].any() or set(rec["flags"]) <= {0, _lib.VIS_QUERIED}
        assert not rec["n_points"].any() and np.array_equal(np.diag(mat), rec["n_visible"].astype(np.uint32))
        assert cnt["elements_counted"] == int(rec["n_visible"].sum())


def test_bad_lists(host):
    tracks, ids, poses, points, mask = random_session(5, T=10)
    vtw.run(host, tracks, ids, poses, points, mask, [ids[0], ids[0]], "map", expect=4)
    vtw.run(host, tracks, ids, poses, points, mask, [2], "map", expect=4)   # (the ids are drawn from 3 .. 59)
