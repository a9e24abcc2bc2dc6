"""The host twin of the feature tracks (monocularsfm_amd/csrc/msfm_tracks.h: node numbering, filter predicate, serial union-find; built
with g++ into libmsfm_host.so, and once on its own with -Wall -Werror) against the independent numpy reference tests/tracks_ref.py, on
hand-made edge sets (tests/tracks_fixtures.py) whose content is asserted on the reference first.  Exact equality everywhere.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tracks_fixtures as fx  # noqa: E402
import tracks_ref  # noqa: E402

HOST = os.path.join(HERE, "..", "monocularsfm_amd", "host")
CSRC = os.path.join(HERE, "..", "monocularsfm_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
    L.host_tracks_build.restype = C.c_int
    return L


def twin(L, ids, rows, lists, min_pair=0, forests=(), **flt):
    """One session of the twin -> (rc, stats, (offsets, image_ids, point_idx, consistent), {id: track ids}, forest)."""
    ids = np.ascontiguousarray(ids, np.int32)
    rows = np.ascontiguousarray(rows, np.int32)
    pairs = np.concatenate([np.asarray(l[0], np.int32).reshape(-1, 2) for l in lists] + [np.zeros((0, 2), np.int32)])
    qt = np.concatenate([np.asarray(l[2], np.int32).reshape(-1, 2)[l[1][0]:l[1][-1]] for l in lists] + [np.zeros((0, 2), np.int32)])
    lens = np.concatenate([np.diff(np.asarray(l[1], np.int64)) for l in lists] + [np.zeros(0, np.int64)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pairs, qt = np.ascontiguousarray(pairs), np.ascontiguousarray(qt)
    n = int(rows.sum())
    fo = np.ascontiguousarray(np.concatenate([np.asarray(f, np.int32) for f in forests]) if forests else np.zeros(1, np.int32))
    counts = np.zeros(12, np.int64)
    cap = max(n, 1)
    o, img, idx = np.zeros(cap + 1, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    cons, tof, forest = np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = L.host_tracks_build(p(ids), p(rows), len(ids), int(min_pair), p(pairs), len(pairs), p(offsets), p(qt), p(fo), len(forests),
                             int(flt.get("min_length", 2)), int(flt.get("max_length", 0)), int(bool(flt.get("keep_inconsistent", False))),
                             p(counts), p(o), p(img), p(idx), p(cons), p(tof), p(forest), C.c_longlong(cap), C.c_longlong(cap))
    stats = dict(zip(tracks_ref.COUNT_KEYS, counts.tolist()))
    if rc != 0:
        return rc, stats, None, None, None
    T, O = stats["tracks_kept"], stats["observations_kept"]
    sid, srows, base = tracks_ref.numbering(ids, rows)
    tids = {int(sid[k]): tof[base[k]:base[k + 1]] for k in range(len(sid))}
    return rc, stats, (o[:T + 1], img[:O], idx[:O], cons[:T]), tids, forest[:n]


def test_header_builds_on_its_own(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "msfm_tracks.h"\nint main() { MsfmTrackTwin t; MsfmTrackNodes n; n.base.assign(1, 0); t.begin(n, 0); '
                   'return (int)t.finish(MsfmTrackFilter{}).offsets.size() - 1; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_the_hand_made_set_holds_what_it_is_meant_to():
    fx.check_hand_reference()


@pytest.mark.parametrize("flt", fx.FILTERS, ids=lambda f: "min%d-max%d-%s" % (f["min_length"], f["max_length"], "all" if f["keep_inconsistent"] else "consistent"))
def test_twin_equals_reference_under_every_filter(host, flt):
    lists = [fx.csr(fx.HAND)]
    want = tracks_ref.build(fx.IDS, fx.ROWS, lists, fx.MIN_PAIR, **flt)
    rc, stats, tracks, tids, _ = twin(host, fx.IDS, fx.ROWS, lists, fx.MIN_PAIR, **flt)
    assert rc == 0 and fx.same_result(stats, tracks, tids, want)
    assert (want["stats"]["tracks_kept"] > 0) and (flt["keep_inconsistent"] or want["consistent"].all())


def test_min_pair_matches_zero_takes_every_pair(host):
    lists = [fx.csr(fx.HAND)]
    want = tracks_ref.build(fx.IDS, fx.ROWS, lists, 0, keep_inconsistent=True)
    rc, stats, tracks, tids, _ = twin(host, fx.IDS, fx.ROWS, lists, 0, keep_inconsistent=True)
    assert rc == 0 and fx.same_result(stats, tracks, tids, want) and stats["pairs_below_min"] == 0


@pytest.mark.parametrize("seed", range(5))
def test_result_is_a_function_of_the_edge_set(host, seed):
    """Pair order, match order and pair orientation do not matter; neither does the order in which the images are declared."""
    want = tracks_ref.build(fx.IDS, fx.ROWS, [fx.csr(fx.HAND)], fx.MIN_PAIR, keep_inconsistent=True)
    perm = np.random.default_rng(seed).permutation(len(fx.IDS))
    lists = [fx.csr(fx.shuffled(fx.HAND, seed))]
    ref2 = tracks_ref.build(fx.IDS[perm], fx.ROWS[perm], lists, fx.MIN_PAIR, keep_inconsistent=True)
    rc, stats, tracks, tids, _ = twin(host, fx.IDS[perm], fx.ROWS[perm], lists, fx.MIN_PAIR, keep_inconsistent=True)
    assert rc == 0 and fx.same_result(stats, tracks, tids, want) and fx.same_result(ref2["stats"], (ref2["offsets"], ref2["image_ids"],
                                                                                                  ref2["point_idx"], ref2["consistent"]), ref2["track_ids"], want)


def test_numbering_by_smallest_node(host):
    _, _, (o, img, idx, _), _, _ = twin(host, fx.IDS, fx.ROWS, [fx.csr(fx.HAND)], fx.MIN_PAIR, keep_inconsistent=True)
    sid, _, base = tracks_ref.numbering(fx.IDS, fx.ROWS)
    node = base[np.searchsorted(sid, img)] + idx
    assert (np.diff(node[o[:-1]]) > 0).all()                       # tracks by ascending first (= smallest) node
    for t in range(len(o) - 1):
        assert (np.diff(node[o[t]:o[t + 1]]) > 0).all()            # elements by ascending node


def test_empty_sessions(host):
    none = np.zeros(0, np.int32)
    empty = (np.zeros((0, 2), np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32))
    for ids, rows, lists in ((none, none, [empty]), (fx.IDS, fx.ROWS, [empty]), (fx.IDS, np.zeros(5, np.int32), [fx.csr(fx.HAND)])):
        want = tracks_ref.build(ids, rows, lists)
        rc, stats, tracks, tids, _ = twin(host, ids, rows, lists)
        assert rc == 0 and fx.same_result(stats, tracks, tids, want) and stats["tracks_kept"] == 0 and list(tracks[0]) == [0]


def test_forests_join_sessions(host):
    """Two sessions that each saw half of the pairs, joined by export / import, equal one session that saw all."""
    want = tracks_ref.build(fx.IDS, fx.ROWS, [fx.csr(fx.HAND)], fx.MIN_PAIR, keep_inconsistent=True)
    a, b = fx.HAND[0::2], fx.HAND[1::2]
    fa = twin(host, fx.IDS, fx.ROWS, [fx.csr(a)], fx.MIN_PAIR)[4]
    rc, stats, tracks, tids, fb = twin(host, fx.IDS, fx.ROWS, [fx.csr(b)], fx.MIN_PAIR, forests=[fa], keep_inconsistent=True)
    assert rc == 0
    for k in ("tracks_total", "tracks_inconsistent", "tracks_kept", "observations_kept", "longest_track"):
        assert stats[k] == want["stats"][k]
    assert np.array_equal(tracks[0], want["offsets"]) and np.array_equal(tracks[1], want["image_ids"]) and np.array_equal(tracks[2], want["point_idx"])
    ref = tracks_ref.build(fx.IDS, fx.ROWS, [fx.csr(b)], fx.MIN_PAIR, keep_inconsistent=True, forests=[fa])
    assert np.array_equal(ref["offsets"], want["offsets"]) and np.array_equal(ref["point_idx"], want["point_idx"])
    assert np.array_equal(tracks_ref.components(len(fb), np.arange(len(fb)), fb.astype(np.int64)), want["label"])
    bad = fa.copy()
    bad[3] = len(bad)
    assert twin(host, fx.IDS, fx.ROWS, [fx.csr(b)], fx.MIN_PAIR, forests=[bad])[0] == 10


def test_numbering_errors(host):
    one = (np.zeros((0, 2), np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32))
    assert twin(host, [1, 2, 1], [3, 3, 3], [one])[0] == 1 + 2                      # twice
    assert twin(host, [1, 10000], [3, 3], [one])[0] == 1 + 1                        # outside [0, MSFM_MAX_IMAGES)
    assert twin(host, [-1], [3], [one])[0] == 1 + 1


def test_random_edge_sets(host):
    """Seeded random sets with long transitive chains and clashes, every filter field in play."""
    rng = np.random.default_rng(2024)
    for trial in range(6):
        n_img = int(rng.integers(2, 9))
        ids = rng.choice(60, n_img, replace=False).astype(np.int32)
        rows = rng.integers(0, 12, n_img).astype(np.int32)
        items = []
        for _ in range(int(rng.integers(1, 30))):
            a, b = rng.choice(np.concatenate([ids, [61]]), 2)
            m = int(rng.integers(0, 7))
            items.append(((int(a), int(b)), [(int(rng.integers(-1, 13)), int(rng.integers(-1, 13))) for _ in range(m)]))
        flt = dict(min_length=int(rng.integers(0, 5)), max_length=int(rng.integers(0, 8)), keep_inconsistent=bool(rng.integers(0, 2)))
        mp = int(rng.integers(0, 4))
        want = tracks_ref.build(ids, rows, [fx.csr(items)], mp, **flt)
        rc, stats, tracks, tids, _ = twin(host, ids, rows, [fx.csr(items)], mp, **flt)
        assert rc == 0 and fx.same_result(stats, tracks, tids, want), trial
