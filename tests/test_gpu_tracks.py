"""The feature tracks on the device (msfm_tracks_*, csrc/msfm_tracks.hip.h) against the independent numpy reference tests/tracks_ref.py.
Every comparison is exact equality of integer arrays; the reference is fed the very lists the matching calls returned.

  * the hand-made edge sets of tests/tracks_fixtures.py through tracks_add, whole and pair by pair, under every filter;
  * lists of real calls: a 24-image capture with shared scene points (fixtures.scene_job) and a byte job with planted duplicates and
    planted clashes (fixtures.dup_job), through match_pairs, match_pairs_verified under models 0, 1, 2 and the model selection, and
    match_pairs_stream, with cuts forced by set_limits so that three sub-batches fold concurrently;
  * the same result from one call / streamed / reversed pair order / two contexts joined by export-import / a second finish;
  * with a session open, the lists, certificate, selection records, two-view records and verification_stats() equal those without;
  * a production-shaped fold: 4.2 M nodes, several million matches, part of them an adversarial edge set (chains, a star);
  * the errors and lifetimes of every entry point.

What the CPU oracles' lists of the two jobs give through tracks_ref.py (min_pair_matches 0, inconsistent tracks kept), so that the
assertions "at least one track of length >= 3" and "at least one inconsistent track" cannot hold on empty output only:
  scene_job (oracle/c_oracle.match_pair, ratio 0.8, cross-check, 0.7): 16 453 edges, 1 456 tracks, 1 337 of length >= 3, longest 12
  dup_job   (oracle/int_oracle.match_pair, 0.8, cross-check, 1e9):     5 280 edges, 80 tracks, all of length >= 3, 3 inconsistent, longest 13
"""
import numpy as np
import pytest

import tracks_fixtures as fx
import tracks_ref
from monocularsfm_amd import _lib

pytestmark = pytest.mark.gpu
CAM = (2500.0, 2500.0, 1536.0, 1152.0)


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def upload(ctx, ids, imgs, kps=None):
    for k, i in enumerate(ids):
        ctx.upload_image(int(i), imgs[k])
        if kps is not None:
            ctx.upload_keypoints(int(i), kps[k])


def upload_rows(ctx, ids, rows, seed=5):
    rng = np.random.default_rng(seed)
    for i, n in zip(ids, rows):
        ctx.upload_image(int(i), rng.integers(0, 256, (int(n), 128), dtype=np.uint8))


def result(ctx, ids, **flt):
    stats = ctx.tracks_finish(**flt)
    return stats, ctx.tracks(), {int(i): ctx.track_ids(int(i)) for i in ids}


def check(ctx, ids, want, **flt):
    stats, tracks, tids = result(ctx, ids, **flt)
    assert fx.same_result(stats, tracks, tids, want)
    assert stats["device_bytes"] >= 4 * stats["nodes"] and stats["finish_ms"] >= 0.0 and stats["fold_ms"] >= 0.0
    return stats


def same_lists(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_hand_made_sets_through_tracks_add(tctx):
    fx.check_hand_reference()
    upload_rows(tctx, fx.IDS, fx.ROWS)
    whole = fx.csr(fx.HAND)
    for split in (False, True):
        tctx.tracks_begin(fx.IDS, min_pair_matches=fx.MIN_PAIR)
        if split:
            for item in fx.HAND:
                tctx.tracks_add(*fx.csr([item]))
        else:
            tctx.tracks_add(*whole)
        for flt in fx.FILTERS:   # finish again and again with another filter: the forest is kept
            want = tracks_ref.build(fx.IDS, fx.ROWS, [whole], fx.MIN_PAIR, **flt)
            check(tctx, fx.IDS, want, **flt)
        tctx.tracks_end()
    # the same set of edges in another order, images declared in another order, every pair
    for seed in range(3):
        lists = fx.csr(fx.shuffled(fx.HAND, seed))
        tctx.tracks_begin(fx.IDS[::-1].copy(), min_pair_matches=0)
        tctx.tracks_add(*lists)
        check(tctx, fx.IDS, tracks_ref.build(fx.IDS, fx.ROWS, [fx.csr(fx.HAND)], 0, keep_inconsistent=True), keep_inconsistent=True)
        tctx.tracks_end()
    # offsets that do not start at 0 address the caller's qt absolutely
    pairs, offsets, qt = whole
    tctx.tracks_begin(fx.IDS, min_pair_matches=fx.MIN_PAIR)
    tctx.tracks_add(pairs[2:], offsets[2:], qt)
    tctx.tracks_add(pairs[:2], offsets[:3], qt)
    check(tctx, fx.IDS, tracks_ref.build(fx.IDS, fx.ROWS, [whole], fx.MIN_PAIR))
    tctx.tracks_end()


def test_empty_sessions(tctx):
    upload_rows(tctx, fx.IDS, fx.ROWS)
    tctx.upload_image(20, np.zeros((0, 128), np.uint8))
    for ids, rows in ((np.zeros(0, np.int32), np.zeros(0, np.int32)), (fx.IDS, fx.ROWS), (np.asarray([20], np.int32), np.asarray([0], np.int32))):
        tctx.tracks_begin(ids)
        st = check(tctx, ids, tracks_ref.build(ids, rows, []))
        assert st["tracks_kept"] == 0 and st["nodes"] == int(rows.sum()) and len(tctx.tracks_export_forest()) == st["nodes"]
        tctx.tracks_end()


def scene(ctx):
    ids, imgs, kps, pairs = fx.scene_job()
    upload(ctx, ids, imgs, kps)
    return ids, [len(x) for x in imgs], pairs


def test_match_pairs_folds_its_lists_and_changes_nothing(tctx):
    ids, rows, pairs = scene(tctx)
    off = tctx.match_pairs(pairs)
    cert_off = tctx.order_certificate(len(pairs))
    tctx.set_limits(max_pairs_per_batch=23)            # 12 sub-batches: three in flight, their folds on three streams
    tctx.tracks_begin(ids)
    on = tctx.match_pairs(pairs)
    assert tctx.profile()["sub_batches"] >= 12
    assert same_lists(on, off) and np.array_equal(tctx.order_certificate(len(pairs)), cert_off)
    q, t, _ = tctx.match_pair(int(pairs[0][0]), int(pairs[0][1]))     # takes no part
    tctx.knn2_pair(int(pairs[0][0]), int(pairs[0][1]))
    want = tracks_ref.build(ids, rows, [(pairs, on[0], on[1])], keep_inconsistent=True)
    st = check(tctx, ids, want, keep_inconsistent=True)
    assert st["edges"] == on[0][-1] and st["pairs"] == len(pairs) and int((np.diff(want["offsets"]) >= 3).sum()) >= 1
    assert st["longest_track"] >= 3 and st["tracks_kept"] > 100
    # after finish a matching call no longer folds; another filter on the kept forest; SceneGraph::Load's threshold in a new session
    tctx.match_pairs(pairs)
    check(tctx, ids, tracks_ref.build(ids, rows, [(pairs, on[0], on[1])], min_length=3, max_length=6), min_length=3, max_length=6)
    tctx.tracks_end()
    tctx.tracks_begin(ids, min_pair_matches=60)
    tctx.match_pairs(pairs[::-1].copy())               # reversed pair order, other cuts
    want60 = tracks_ref.build(ids, rows, [(pairs, on[0], on[1])], 60)
    st = check(tctx, ids, want60)
    assert 0 < st["pairs_below_min"] < len(pairs)
    tctx.tracks_end()
    assert same_lists(tctx.match_pairs(pairs), off)


@pytest.mark.parametrize("model,select", [(0, False), (1, False), (2, False), (0, True), (1, True)])
def test_verified_calls_fold_the_lists_they_hand_out(tctx, model, select):
    ids, rows, pairs = scene(tctx)
    tctx.set_verification_model(model, CAM if model == 1 else None)
    tctx.set_model_selection(select)
    if model == 1:
        tctx.set_two_view_geometry(True, min_num_inliers=20)
    tctx.set_limits(max_pairs_per_batch=40)
    off = tctx.match_pairs_verified(pairs)
    stats_off = tctx.verification_stats()
    sel_off = tctx.model_selection(len(pairs)) if select else None
    tv_off = tctx.two_view_geometry(len(pairs)).copy() if model == 1 else None
    tctx.tracks_begin(ids)
    on = tctx.match_pairs_verified(pairs)
    assert same_lists(on, off) and tctx.verification_stats() == stats_off
    if select:
        assert same_lists(tctx.model_selection(len(pairs)), sel_off)
    if model == 1:
        assert tctx.two_view_geometry(len(pairs)).tobytes() == tv_off.tobytes()
    want = tracks_ref.build(ids, rows, [(pairs, on[0], on[1])], keep_inconsistent=True)
    st = check(tctx, ids, want, keep_inconsistent=True)
    assert st["edges"] == on[0][-1] > 0 and int((np.diff(want["offsets"]) >= 3).sum()) >= 1
    tctx.tracks_end()
    # the verified streaming form: every chunk folds as it is handed out
    tctx.tracks_begin(ids)
    chunks = [(pairs[c["first"]:c["first"] + c["n_pairs"]], c["offsets"], c["qt"]) for c in tctx.match_pairs_stream(pairs, verified=True)]
    assert len(chunks) >= 3 and np.array_equal(np.concatenate([c[2] for c in chunks]), on[1])
    check(tctx, ids, tracks_ref.build(ids, rows, chunks, keep_inconsistent=True), keep_inconsistent=True)
    check(tctx, ids, want, keep_inconsistent=True)
    tctx.tracks_end()


def test_duplicates_clashes_streams_and_two_contexts(tctx):
    ids, imgs, pairs = fx.dup_job()
    rows = [len(x) for x in imgs]
    upload(tctx, ids, imgs)
    prm = dict(ratio=0.8, cross_check=True, max_distance=1e9)
    tctx.set_limits(max_pairs_per_batch=7)
    tctx.tracks_begin(ids)
    one = tctx.match_pairs(pairs, **prm)
    want = tracks_ref.build(ids, rows, [(pairs, one[0], one[1])], keep_inconsistent=True)
    st = check(tctx, ids, want, keep_inconsistent=True)
    assert st["tracks_inconsistent"] >= 1 and st["longest_track"] >= 3
    st2 = check(tctx, ids, tracks_ref.build(ids, rows, [(pairs, one[0], one[1])]))       # a second finish: consistent tracks only
    assert st2["tracks_kept"] == st["tracks_kept"] - st["tracks_inconsistent"]
    tctx.tracks_end()
    # streamed
    tctx.tracks_begin(ids)
    n_chunks = sum(1 for _ in tctx.match_pairs_stream(pairs, **prm))
    assert n_chunks >= 9
    check(tctx, ids, want, keep_inconsistent=True)
    tctx.tracks_end()
    # reversed pair order
    tctx.tracks_begin(ids)
    tctx.match_pairs(pairs[::-1].copy(), **prm)
    check(tctx, ids, want, keep_inconsistent=True)
    tctx.tracks_end()
    # two contexts, each half of the pairs, joined by export / import (the one-context-per-GPU fan-out)
    other = _lib.Context(0)
    try:
        upload(other, ids, imgs)
        other.set_limits(max_pairs_per_batch=5)
        tctx.tracks_begin(ids)
        other.tracks_begin(ids[::-1].copy())
        a = tctx.match_pairs(pairs[0::2].copy(), **prm)
        b = other.match_pairs(pairs[1::2].copy(), **prm)
        forest = other.tracks_export_forest()
        assert len(forest) == sum(rows) and forest.min() >= 0 and forest.max() < sum(rows)
        half = tracks_ref.build(ids, rows, [(pairs[1::2], b[0], b[1])], keep_inconsistent=True)
        assert np.array_equal(tracks_ref.components(len(forest), np.arange(len(forest)), forest.astype(np.int64)), half["label"])
        tctx.tracks_import_forest(forest)
        stats, tracks, tids = result(tctx, ids, keep_inconsistent=True)
        assert same_lists(tracks, (want["offsets"], want["image_ids"], want["point_idx"], want["consistent"]))
        assert all(np.array_equal(tids[int(i)], want["track_ids"][int(i)]) for i in ids)
        assert stats["edges"] == a[0][-1] and stats["tracks_inconsistent"] == want["stats"]["tracks_inconsistent"]
        other.tracks_end()
        tctx.tracks_end()
    finally:
        other.close()


def test_production_shaped_fold(tctx):
    """512 images x 8192 rows = 4 194 304 nodes: a 16 MiB forest, four times one XCD's L2.  Real lists: every image is a row permutation
    of one base image with one byte changed, so each of 384 matched pairs keeps 8192 matches (3.1 M edges through match_pairs, cut into
    sub-batches that fold concurrently).  Adversarial lists through tracks_add: 64 chains that run through every image in a scrambled
    order (long paths: 32 704 edges whose unions arrive out of order) and a star of 1 M edges on one node (contended compare-and-swap
    on one root's word)."""
    n_img, n = 512, 8192
    rng = np.random.default_rng(99)
    base = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    ids = np.arange(n_img, dtype=np.int32) * 3
    for k in range(n_img):
        d = base[rng.permutation(n)]
        d[:, k % 128] ^= 1
        tctx.upload_image(int(ids[k]), d)
    rows = [n] * n_img
    real = np.stack([ids[(np.arange(384) * 7) % n_img], ids[(np.arange(384) * 7 + 1 + np.arange(384) % 5) % n_img]], 1).astype(np.int32)
    tctx.set_limits(max_pairs_per_batch=48)
    tctx.tracks_begin(ids, min_pair_matches=10)
    got = tctx.match_pairs(real, max_distance=1e9)
    assert got[0][-1] >= 3_000_000 and tctx.profile()["sub_batches"] >= 8
    order = rng.permutation(n_img)
    chain_pairs = np.stack([ids[order[:-1]], ids[order[1:]]], 1).astype(np.int32)
    chain_rows = rng.integers(0, n, (n_img, 64))
    chain_qt = np.stack([chain_rows[order[:-1]], chain_rows[order[1:]]], 2).reshape(-1, 2).astype(np.int32)
    chain = (chain_pairs, np.arange(n_img, dtype=np.int64) * 64, chain_qt)
    shuffle = rng.permutation(n_img - 1)                      # the chains' links in a scrambled order
    chain = (chain[0][shuffle], chain[1], chain_qt.reshape(n_img - 1, 64, 2)[shuffle].reshape(-1, 2))
    star_pairs = np.stack([np.full(n_img - 1, ids[5]), np.delete(ids, 5)], 1).astype(np.int32)
    per = 2048
    star_qt = np.stack([np.full((n_img - 1) * per, 17), rng.integers(0, n, (n_img - 1) * per)], 1).astype(np.int32)
    star = (star_pairs, np.arange(n_img, dtype=np.int64) * per, star_qt)
    tctx.tracks_add(*chain)
    tctx.tracks_add(*star)
    lists = [(real, got[0], got[1]), chain, star]
    want = tracks_ref.build(ids, rows, lists, 10, keep_inconsistent=True)
    st = check(tctx, ids[::37], want, keep_inconsistent=True)
    assert st["nodes"] == n_img * n >= 4_000_000 and st["edges"] >= 4_000_000
    assert st["longest_track"] >= 1_000_000 and st["tracks_inconsistent"] >= 1
    check(tctx, ids[::37], tracks_ref.build(ids, rows, lists, 10, max_length=n_img), max_length=n_img)
    tctx.tracks_end()


def test_errors_and_lifetimes(tctx):
    E = _lib

    def code(fn, *a, **k):
        with pytest.raises(_lib.MsfmError) as e:
            fn(*a, **k)
        return e.value.code

    upload_rows(tctx, fx.IDS, fx.ROWS)
    one = fx.csr(fx.HAND[:1])
    # no session: everything but begin / end is a state error
    assert code(tctx.tracks_add, *one) == E.E_STATE and code(tctx.tracks_finish) == E.E_STATE and code(tctx.tracks) == E.E_STATE
    assert code(tctx.track_ids, 3) == E.E_STATE and code(tctx.tracks_import_forest, np.zeros(29, np.int32)) == E.E_STATE
    assert tctx._L.msfm_tracks_export_forest(tctx._h, None) == E.E_STATE
    tctx.tracks_end()                                           # no session: nothing happens
    # begin: bad lists
    assert code(tctx.tracks_begin, [3, 5, 3]) == E.E_INVALID
    assert code(tctx.tracks_begin, [3, 10000]) == E.E_INVALID and code(tctx.tracks_begin, [-1]) == E.E_INVALID
    assert code(tctx.tracks_begin, [3, 4]) == E.E_NOIMAGE
    assert code(tctx.tracks_begin, [3], min_pair_matches=-1) == E.E_INVALID
    assert tctx._L.msfm_tracks_begin(tctx._h, None, 2, None) == E.E_INVALID
    # begin while a streaming series is open
    gen = tctx.match_pairs_stream([(3, 5), (5, 7)], max_distance=1e9)
    tctx.set_limits(max_pairs_per_batch=1)
    next(gen)
    assert code(tctx.tracks_begin, fx.IDS) == E.E_STATE
    gen.close()
    tctx.tracks_begin(fx.IDS)
    assert code(tctx.tracks_begin, fx.IDS) == E.E_STATE           # a session is open
    # fetch before finish
    assert code(tctx.tracks) == E.E_STATE and code(tctx.track_ids, 3) == E.E_STATE
    # the declared images cannot change; others can
    assert code(tctx.clear_images) == E.E_STATE
    assert code(tctx.upload_image, 3, np.zeros((4, 128), np.uint8)) == E.E_STATE
    assert code(tctx.subset_image, 5, 3, [0, 1]) == E.E_STATE
    tctx.upload_image(40, np.zeros((4, 128), np.uint8))
    tctx.subset_image(3, _lib.MAX_IMAGES + 3, [0, 1])
    # add: bad arguments are errors, bad matches are not
    assert tctx._L.msfm_tracks_add(tctx._h, None, 1, None, None) == E.E_INVALID
    bad = np.asarray([0, 3, 2], np.int64)
    assert tctx._L.msfm_tracks_add(tctx._h, one[0].ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), 2,
                                   bad.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64)), one[2].ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))) == E.E_INVALID
    tctx.tracks_add(*one)
    # import: an entry outside [0, nodes) joins nothing
    forest = tctx.tracks_export_forest()
    with pytest.raises(ValueError):
        tctx.tracks_import_forest(forest[:-1])                    # the binding checks the length before the library reads it
    wrong = forest.copy()
    wrong[-1] = len(forest)
    assert code(tctx.tracks_import_forest, wrong) == E.E_INVALID
    wrong[-1] = -1
    assert code(tctx.tracks_import_forest, wrong) == E.E_INVALID
    # finish while a series is open
    gen = tctx.match_pairs_stream([(3, 5), (5, 7)], max_distance=1e9)
    next(gen)
    assert code(tctx.tracks_finish) == E.E_STATE
    gen.close()
    assert code(tctx.tracks_finish, max_length=-1) == E.E_INVALID
    st = tctx.tracks_finish()
    assert st["tracks_kept"] >= 3
    assert code(tctx.track_ids, 40) == E.E_INVALID                # resident, not declared
    # after finish: no more accumulation, the result stays until end
    assert code(tctx.tracks_add, *one) == E.E_STATE and code(tctx.tracks_import_forest, forest) == E.E_STATE
    again = tctx.tracks()
    tctx.match_pairs([(3, 5)])
    assert same_lists(tctx.tracks(), again)
    tctx.tracks_end()
    assert code(tctx.tracks) == E.E_STATE
    tctx.clear_images()                                         # the store is free again
    # NULL outputs where the header allows them
    upload_rows(tctx, fx.IDS, fx.ROWS)
    tctx.tracks_begin(fx.IDS)
    tctx.tracks_add(*fx.csr(fx.HAND))
    assert tctx._L.msfm_tracks_finish(tctx._h, None, None) == E.OK
    assert tctx._L.msfm_fetch_tracks(tctx._h, None, None, None, None) == E.OK
    # a context destroyed with a session open frees it (nothing to assert but the absence of a fault)
