"""Hand-made edge sets for the feature tracks and the comparison against tests/tracks_ref.py, shared by the host-twin test and the GPU
tests.  Test infrastructure only."""
import itertools

import numpy as np

import tracks_ref

# images in NON-ascending order of id on purpose: the numbering ranks them by id
IDS = np.asarray([7, 3, 12, 5, 9], np.int32)
ROWS = np.asarray([8, 6, 6, 5, 4], np.int32)          # rows of 7, 3, 12, 5, 9
MIN_PAIR = 2

# (id1, id2) -> (q, t) matches; listed in this order (a pair may come twice)
HAND = [
    ((3, 5), [(0, 0), (1, 1), (5, 4)]),               # a - b
    ((5, 7), [(0, 0), (2, 2), (4, 7)]),               # b - c: (3, 0) and (7, 0) are never matched, the track is transitive
    ((3, 7), [(1, 3), (2, 4)]),
    ((7, 9), [(5, 0), (6, 0), (7, 3)]),               # two keypoints of image 7 on one of image 9: an inconsistent track
    ((3, 5), [(0, 0), (1, 1), (5, 4)]),               # the first pair once more: idempotent
    ((5, 9), [(3, 1), (1, 2)]),
    ((3, 12), [(3, 1), (4, 2), (5, 99), (-1, 0)]),    # two indices out of range: ignored
    ((9, 12), [(1, 1)]),                              # below MIN_PAIR: would merge the tracks of (5, 3)-(9, 1) and (3, 3)-(12, 1)
    ((7, 7), [(0, 1), (1, 2)]),                       # a self pair: ignored
    ((3, 10007), [(0, 0), (1, 1)]),                   # the pre-emptive filter's subset image: skipped
    ((4, 3), [(0, 0), (1, 1)]),                       # an image that was never declared: skipped
    ((7, 12), [(7, 5), (0, 0)]),                      # closes the chain 3:5 - 5:4 - 7:7 - 9:3 - 12:5 (length 5)
    ((12, 9), []),                                    # an empty list (below MIN_PAIR as well)
]


def csr(items):
    pairs = np.asarray([p for p, _ in items], np.int32).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([len(m) for _, m in items])]).astype(np.int64)
    flat = [m for _, ms in items for m in ms]
    qt = np.asarray(flat, np.int32).reshape(-1, 2)
    return pairs, offsets, qt


def shuffled(items, seed):
    """The same SET of edges: pairs in another order, the matches of each in another order, some pairs given as (id2, id1)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in rng.permutation(len(items)):
        (a, b), ms = items[k]
        ms = [ms[i] for i in rng.permutation(len(ms))]
        if rng.random() < 0.5:
            (a, b), ms = (b, a), [(t, q) for q, t in ms]
        out.append(((a, b), ms))
    return out


FILTERS = [dict(min_length=a, max_length=b, keep_inconsistent=c) for a, b, c in itertools.product((0, 2, 3), (0, 4), (False, True))]


def same_result(stats, tracks, track_ids, want):
    """stats dict, (offsets, image_ids, point_idx, consistent), {image id: ids} against a tracks_ref.build() result: exact equality."""
    for k in tracks_ref.COUNT_KEYS:
        assert int(stats[k]) == int(want["stats"][k]), (k, stats[k], want["stats"][k])
    offsets, image_ids, point_idx, consistent = tracks
    assert np.array_equal(np.asarray(offsets, np.int64), want["offsets"])
    assert np.array_equal(np.asarray(image_ids, np.int32), want["image_ids"])
    assert np.array_equal(np.asarray(point_idx, np.int32), want["point_idx"])
    assert np.array_equal(np.asarray(consistent, np.uint8), want["consistent"])
    for i, got in track_ids.items():          # (every declared image, or the sample of them the caller fetched)
        assert np.array_equal(np.asarray(got, np.int32), want["track_ids"][int(i)]), i
    return True


def track_sets(res):
    """A result as a list of frozensets of (image id, keypoint) -- for assertions about what a fixture contains."""
    o = res["offsets"]
    return [frozenset(zip(res["image_ids"][o[t]:o[t + 1]].tolist(), res["point_idx"][o[t]:o[t + 1]].tolist())) for t in range(len(o) - 1)]


def check_hand_reference():
    """What the hand-made set is meant to contain, asserted on the reference alone."""
    everything = tracks_ref.build(IDS, ROWS, [csr(HAND)], MIN_PAIR, keep_inconsistent=True)
    sets = track_sets(everything)
    assert frozenset({(3, 0), (5, 0), (7, 0), (12, 0)}) in sets                     # transitive
    assert frozenset({(7, 5), (7, 6), (9, 0)}) in sets                              # inconsistent
    assert frozenset({(3, 5), (5, 4), (7, 7), (9, 3), (12, 5)}) in sets             # the chain of five
    assert frozenset({(5, 3), (9, 1)}) in sets and frozenset({(3, 3), (12, 1)}) in sets   # kept apart by MIN_PAIR
    st = everything["stats"]
    assert st["tracks_inconsistent"] == 1 and st["pairs_below_min"] == 2 and st["pairs_skipped"] == 2
    assert st["matches_ignored"] == 4 and st["pairs"] == 8 and st["tracks_total"] == 9 and st["longest_track"] == 5
    merged = tracks_ref.build(IDS, ROWS, [csr(HAND)], 0, keep_inconsistent=True)
    assert frozenset({(5, 3), (9, 1), (3, 3), (12, 1)}) in track_sets(merged)       # ... and only by it
    capped = tracks_ref.build(IDS, ROWS, [csr(HAND)], MIN_PAIR, max_length=4, keep_inconsistent=True)
    assert capped["stats"]["tracks_over_max_length"] == 1 and capped["stats"]["tracks_kept"] == 8
    # numbering by smallest node: image 3 is rank 0, so its keypoints 0, 1, 2, .. open the first tracks
    assert everything["image_ids"][everything["offsets"][:-1]].tolist() == sorted(everything["image_ids"][everything["offsets"][:-1]].tolist())
    return everything


def scene_job(n_images=24, n_desc=600, n_proto=1500, seed=77):
    """A capture of a few dozen images that share scene points: RootSIFT-like rows drawn from one prototype pool, keypoints that observe
    the prototypes' 3-D points through synth.scene_cameras.  -> (ids, descriptors, keypoints, all pairs as ids)."""
    from monocularsfm_amd import synth
    imgs, protos = synth.rootsift_images(n_images, n_desc, seed=seed, n_proto=n_proto, return_proto=True)
    cams = synth.scene_cameras(n_images, seed=seed)
    kps = synth.scene_keypoints(protos, cams, n_proto, seed=seed)
    ids = np.asarray([3 * i + 1 for i in range(n_images)], np.int32)
    return ids, imgs, kps, ids[synth.all_pairs(n_images)]


def dup_job(n_images=12, n_desc=400, seed=43, n_clash=3):
    """synth.u8_images with planted duplicates (every image carries a noisy copy of every pool row: tracks through all images), and
    n_clash planted CLASHES: image 0 gets a second row a' = a + e beside its copy a of a pool row, image 2's copy becomes a + e too.
    Then a matches the other images' copies, a' matches image 2's, and image 2's matches the other images': one component with two
    keypoints of image 0 -- an inconsistent track.  -> (ids, descriptors uint8, all pairs as ids)."""
    from monocularsfm_amd import synth
    imgs, planted = synth.u8_images(n_images, n_desc, seed=seed, dup_frac=0.2, as_float=False, return_planted=True)
    rng = np.random.default_rng(seed + 1)
    free = np.setdiff1d(np.arange(n_desc), planted[0])
    for k in range(n_clash):
        a = imgs[0][planted[0][k]].astype(np.int64)
        e = np.rint(rng.normal(0.0, 12.0, 128)).astype(np.int64)
        imgs[0][free[k]] = np.clip(a + e, 0, 255).astype(np.uint8)
        imgs[2][planted[2][k]] = np.clip(a + e + np.rint(rng.normal(0.0, 1.0, 128)).astype(np.int64), 0, 255).astype(np.uint8)
    ids = np.asarray([2 * i for i in range(n_images)], np.int32)
    return ids, imgs, ids[synth.all_pairs(n_images)]
