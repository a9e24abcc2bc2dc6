"""Vocabulary retrieval (matching mode 2) on the GPU against the numpy reference (tests/retrieval_ref.py): the nearest word of every row
bit for bit, the trained centroids byte for byte, the scores within the documented bound and bit-stable, the selection."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import retrieval_ref as ref  # noqa: E402

from monocularsfm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _fresh(ctx, images):
    ctx.clear_images()
    for i, x in images.items():
        ctx.upload_image(i, x)


def _edge_images(rng):
    imgs = {}
    for k, n in enumerate([0, 1, 511, 512, 513]):
        imgs[k] = rng.integers(0, 256, size=(n, 128)).astype(np.uint8)
    imgs[5] = rng.integers(0, 256, size=(300, 128)).astype(np.float32)            # f32 holding integers: q = x
    unit = rng.random((300, 128)).astype(np.float32)
    unit[:40] = (rng.integers(0, 255, size=(40, 128)) + 0.5).astype(np.float32) / np.float32(255.0)   # x 255 near .5
    unit[40:60] = np.float32(0.5) / np.float32(255.0) * (2 * rng.integers(0, 128, size=(20, 128)) + 1).astype(np.float32)
    imgs[6] = unit
    edge = np.zeros((64, 128), np.uint8)
    edge[32:] = 255                                                                # all-0 and all-255 rows
    imgs[7] = edge
    return imgs


@pytest.mark.parametrize("v", [1, 33, 1000, 16384])
def test_image_words_bit_for_bit(ctx, v):
    rng = np.random.default_rng(100 + v)
    imgs = _edge_images(rng)
    words = rng.integers(0, 256, size=(v, 128)).astype(np.uint8)
    if v >= 33:
        words[v // 2] = words[3]          # duplicate centroids: the lower word wins
    if v == 16384:
        words[9000] = words[100]          # ... across the 8192-word passes as well
        imgs[8] = np.repeat(words[[100, 9000, 3]], 5, axis=0)
    _fresh(ctx, imgs)
    ctx.set_vocabulary(words)
    for i, x in imgs.items():
        got = ctx.image_words(i)
        want = ref.assign(ref.quantize(x), words)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (i, v, np.flatnonzero(got != want)[:5])


def test_equidistant_rows_take_the_lower_word(ctx):
    rng = np.random.default_rng(7)
    words = rng.integers(0, 256, size=(200, 128)).astype(np.uint8)
    base = rng.integers(10, 240, size=128)
    words[150] = base
    words[40] = base
    words[40, 5] += 2
    words[150, 5] -= 0       # word 150 = base, word 40 = base + 2 e5: a row at base + 1 e5 is equidistant from both
    row = base.copy()
    row[5] += 1
    x = np.repeat(row[None, :], 70, axis=0).astype(np.uint8)
    _fresh(ctx, {0: x})
    ctx.set_vocabulary(words)
    got = ctx.image_words(0)
    assert np.all(got == 40)
    assert np.array_equal(got, ref.assign(ref.quantize(x), words))


def test_train_vocabulary_byte_for_byte(ctx):
    rng = np.random.default_rng(11)
    imgs = {i: rng.integers(0, 256, size=(n, 128)).astype(np.uint8) for i, n in enumerate([700, 0, 513, 900, 64])}
    # duplicate rows so that two initial words coincide: the second stays empty and keeps its centroid
    imgs[2][:] = imgs[2][0]
    ids = [3, 0, 4, 2, 1]
    _fresh(ctx, imgs)
    for v, t, m in [(33, 8, 1000), (20, 3, 0), (300, 8, 2179)]:
        want, _ = ref.train(imgs, ids, num_words=v, iters=t, max_rows=m if m else None)
        got = ctx.train_vocabulary(ids, num_words=v, train_iters=t, train_rows=m)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (v, t, m)
    # an empty word was planted in the last case: two identical initial words
    order, q, _ = ref.concat(imgs, ids)
    s, ms = ref.sample_plan(len(q), 2179)
    smp = q[0:s * ms:s][:ms]
    init = smp[ref.initial_rows(ref.vocab_size(300, ms), ms)]
    assert len(np.unique(init, axis=0)) < len(init)


def test_train_on_float_images(ctx):
    rng = np.random.default_rng(12)
    imgs = {i: rng.random((400, 128)).astype(np.float32) for i in range(4)}
    _fresh(ctx, imgs)
    want, _ = ref.train(imgs, list(imgs), num_words=40, iters=5)
    assert np.array_equal(ctx.train_vocabulary(list(imgs), num_words=40, train_iters=5), want)


@pytest.fixture(scope="module")
def scene():
    images, overlap = ref.covis_scene(40, window=8, stride=2, seed=5)
    words, _ = ref.train(images, list(images), num_words=256, iters=8)   # more words than the scene's 86 prototypes
    order, s, nnz = ref.scores(images, list(images), words)
    return images, overlap, words, order, s, nnz


def test_scores_bound_bits_symmetry(ctx, scene):
    images, _, words, order, s, nnz = scene
    _fresh(ctx, images)
    ctx.set_vocabulary(words)
    _, _, m1 = ctx.retrieve_pairs(order, 5, score_matrix=True)
    _, _, m2 = ctx.retrieve_pairs(order, 5, score_matrix=True)
    perm = np.random.default_rng(1).permutation(len(order))
    _, _, m3 = ctx.retrieve_pairs([order[p] for p in perm], 5, score_matrix=True)
    assert np.array_equal(m1.view(np.int32), m2.view(np.int32))
    assert np.array_equal(m1.view(np.int32), m1.T.view(np.int32))
    assert np.array_equal(m3.view(np.int32), m1[np.ix_(perm, perm)].view(np.int32))
    bound = ref.score_bound(nnz[:, None], nnz[None, :])
    err = np.abs(m1.astype(np.float64) - s)
    assert np.all(err <= bound), float((err / bound).max())


def test_selection_equals_reference_away_from_ties(ctx, scene):
    images, _, words, order, s, nnz = scene
    _fresh(ctx, images)
    ctx.set_vocabulary(words)
    k = 5
    pairs, scores, m = ctx.retrieve_pairs(order, k, score_matrix=True)
    got = {tuple(p) for p in pairs.tolist()}
    bound = ref.score_bound(nnz[:, None], nnz[None, :]).max()
    checked = 0
    for a, i in enumerate(order):
        srt = np.sort(s[a][s[a] > 0])[::-1]
        if len(srt) > k and srt[k - 1] - srt[k] <= 2 * bound:
            continue
        for j in (order[b] for b in ref.topk(s[a], order, a, k)):
            assert (max(i, j), min(i, j)) in got
        checked += 1
    assert checked >= len(order) // 2
    # the device selection is exactly the reference rule applied to the device scores
    assert sorted(got) == ref.select(m, order, k)
    assert pairs.tolist() == sorted(pairs.tolist())
    assert all(a > b for a, b in pairs.tolist())
    for (a, b), sc in zip(pairs.tolist(), scores):
        assert sc == m[order.index(a), order.index(b)]


def test_recall_on_planted_scene(ctx, scene):
    images, overlap, words, order, _, _ = scene
    _fresh(ctx, images)
    ctx.set_vocabulary(words)
    pairs, _ = ctx.retrieve_pairs(order, 6)
    got = {tuple(p) for p in pairs.tolist()}
    for i in order:
        for j in order:
            if i > j and overlap(i, j) >= 0.5:
                assert (i, j) in got


def test_k_at_least_n_minus_1_gives_every_positive_pair(ctx, scene):
    images, _, words, order, _, _ = scene
    _fresh(ctx, images)
    ctx.set_vocabulary(words)
    pairs, _, m = ctx.retrieve_pairs(order, len(order) - 1, score_matrix=True)
    want = sorted((max(order[a], order[b]), min(order[a], order[b])) for a in range(len(order)) for b in range(a) if m[a, b] > 0)
    assert [tuple(p) for p in pairs.tolist()] == want


def test_duplicate_images_tie_to_the_lower_id(ctx):
    rng = np.random.default_rng(21)
    a = rng.integers(0, 128, size=(300, 128)).astype(np.uint8)      # two distributions: words of their own
    b = rng.integers(128, 256, size=(300, 128)).astype(np.uint8)
    imgs = {0: a, 5: b.copy(), 3: b.copy(), 9: b.copy(), 7: a.copy()}
    _fresh(ctx, imgs)
    ctx.train_vocabulary(list(imgs), num_words=32)
    pairs, scores, m = ctx.retrieve_pairs([9, 0, 3, 7, 5], 1, score_matrix=True)
    got = {tuple(p) for p in pairs.tolist()}
    # 5 and 9 each take 3 (the lowest of their exact twins), 3 takes 5; 0 and 7 take each other
    assert got == {(5, 3), (9, 3), (7, 0)}
    ix = {i: p for p, i in enumerate([9, 0, 3, 7, 5])}
    assert m[ix[5], ix[3]] == m[ix[5], ix[9]] == m[ix[3], ix[9]] > 0


def test_errors_leave_the_context_usable(ctx):
    rng = np.random.default_rng(31)
    x0 = rng.integers(0, 256, size=(100, 128)).astype(np.uint8)
    with _lib.Context(0) as c:
        c.upload_image(0, x0)
        c.upload_image(1, rng.integers(0, 256, size=(100, 128)).astype(np.uint8))
        # no vocabulary
        for call in (lambda: c.retrieve_pairs([0, 1], 5), lambda: c.image_words(0)):
            with pytest.raises(_lib.MsfmError) as e:
                call()
            assert e.value.code == _lib.E_STATE
        # an unsupported image is named
        c.upload_image(2, np.full((10, 128), 3.5, np.float32))
        with pytest.raises(_lib.MsfmError) as e:
            c.train_vocabulary([0, 2], num_words=4)
        assert e.value.code == _lib.E_INVALID and "image 2" in str(e.value)
        # twice, not resident, too many
        for bad in ([0, 0], [0, 4], list(range(10001))):
            with pytest.raises(_lib.MsfmError) as e:
                c.train_vocabulary(bad, num_words=4)
            assert e.value.code == _lib.E_INVALID
        w = c.train_vocabulary([0, 1], num_words=4)
        for k in (0, 1025):
            with pytest.raises(_lib.MsfmError) as e:
                c.retrieve_pairs([0, 1], k)
            assert e.value.code == _lib.E_INVALID
        with pytest.raises(_lib.MsfmError) as e:
            c.retrieve_pairs([0, 1, 2], 1)
        assert e.value.code == _lib.E_INVALID
        # a streaming series open: the store's users refuse, as the uploads do
        assert c._L.msfm_match_pairs_begin(c._h, _lib._ip(np.array([1, 0], np.int32)), 1, None, 0, None) == _lib.OK
        with pytest.raises(_lib.MsfmError) as e:
            c.retrieve_pairs([0, 1], 1)
        assert e.value.code == _lib.E_STATE
        assert c._L.msfm_match_pairs_end(c._h) == _lib.OK
        # still usable: the vocabulary of the last good training, matching as before
        assert np.array_equal(c.image_words(0), ref.assign(x0, w))
        pairs, _ = c.retrieve_pairs([0, 1], 1)
        assert pairs.shape[1] == 2
        q, t, _ = c.match_pair(0, 1)
        assert len(q) == len(t)
