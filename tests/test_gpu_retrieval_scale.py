"""Vocabulary retrieval (matching mode 2) on the GPU at the shapes it is built for, against the numpy reference (tests/retrieval_ref.py):
scores across many 64 x 64 tiles (ragged last tile, mirrored stores, empty and zero-vector images), top-K at its loop and sort edges,
exact ties among hundreds of identical images, the 10000-image cap, the nearest word beyond two 8192-word passes, training at a larger
shape and the executable beyond one score tile.  Everything is synthetic and seeded.

Most images are exact copies of distinct words, so their nearest words are known in closed form; the device words are checked first,
then the device scores against fp64 scores formed from those words."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import retrieval_ref as ref  # noqa: E402

from monocularsfm_amd import _lib, database, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def _upload(ctx, images, idmap=None):
    ctx.clear_images()
    for i, x in images.items():
        ctx.upload_image(i if idmap is None else int(idmap[i]), x)


def _bits(m):
    return np.ascontiguousarray(m).view(np.int32)


class Scene:
    """n images at ids 0 .. n-1 over V random words.  General images draw their rows from a topic (they all hold the topic's first
    word) plus a few words at random; hubs hold every topic's first word; a cluster's images share private words only, so each has
    exactly size - 1 candidates.  Special images: empty ones between non-empty ones, an all-zero float image, a float image of 0.0 and
    1.0 only (q = x); without empty images every non-empty image also holds the word of the all-zero row, whose idf is then 0, and one
    byte image holds only that word (a zero tf-idf vector, no candidates)."""

    def __init__(self, n, v, seed, empties, clusters=(), hubs=3):
        rng = np.random.default_rng(seed)
        self.n, self.v = n, v
        self.words = rng.integers(0, 256, size=(v, 128)).astype(np.uint8)
        assert len(np.unique(self.words, axis=0)) == v
        self.wz = int(ref.assign(np.zeros((1, 128), np.int64), self.words)[0])   # the word of an all-zero row
        free = rng.permutation(np.setdiff1d(np.arange(v), [self.wz]))
        pools = [free[8 * c:8 * c + 8] for c in range(len(clusters))]
        general = free[8 * len(clusters):]
        pos = rng.permutation(n)
        roles = {}
        special = ["zero", "binary"] + (["empty"] * 3 if empties else ["idf0"])
        for p in (1, n // 2, n - 2, n // 3, 2 * n // 3)[:len(special)]:
            roles[int(p)] = special.pop()
        for c, size in enumerate(clusters):
            take = [int(p) for p in pos if int(p) not in roles][:size]
            for p in take:
                roles[p] = ("cluster", c)
        rest = [p for p in range(n) if p not in roles]
        for p in rest[:hubs]:
            roles[p] = "hub"
        n_topics = max(3, n // 40)
        tp = max(4, min(64, len(general) // (2 * n_topics)))
        topics = [general[t * tp:(t + 1) * tp] for t in range(n_topics)]
        self.images, self.expect = {}, {}
        for p in range(n):
            role = roles.get(p, "general")
            idx = None
            if role == "empty":
                x = np.zeros((0, 128), np.uint8 if p % 2 else np.float32)
            elif role == "zero":
                x = np.zeros((int(rng.integers(1, 20)), 128), np.float32)
            elif role == "binary":
                x = rng.integers(0, 2, size=(int(rng.integers(2, 20)), 128)).astype(np.float32)
                x[0] = 0.0                                      # holds the all-zero row's word as well
            elif role == "idf0":
                idx = np.full(int(rng.integers(1, 10)), self.wz)
            else:
                if role == "hub":
                    idx = np.array([t[0] for t in topics])
                elif isinstance(role, tuple):
                    pool = pools[role[1]]
                    idx = np.concatenate([[pool[0]], rng.choice(pool, size=int(rng.integers(1, 12)))])
                else:
                    t = topics[int(rng.integers(n_topics))]
                    r = int(rng.integers(1, 30))
                    idx = np.concatenate([[t[0]], rng.choice(t, size=r), rng.choice(general, size=int(rng.integers(0, 4)))])
                if not empties:
                    idx = np.concatenate([idx, [self.wz]])
                idx = rng.permutation(idx)
            if idx is not None:
                x = self.words[idx]
                if p % 3 == 1:
                    x = x.astype(np.float32) / np.float32(255.0)   # [0, 1] floats: q = rint(255 x) gives the word back
                self.expect[p] = idx.astype(np.int64)
            else:
                self.expect[p] = ref.assign(ref.quantize(x), self.words)
            self.images[p] = x
        self.roles = [roles.get(p, "general") for p in range(n)]
        self.order = list(range(n))

    def reference(self, ctx, rows=None):
        """device words == the planted words; fp64 S (or its rows `rows`) from them -> (S, nnz)"""
        for p in range(self.n):
            got = ctx.image_words(p)
            assert np.array_equal(got, self.expect[p]), (p, self.roles[p])
        return ref.scores_from_words([self.expect[p] for p in range(self.n)], self.v, rows=rows)


_scenes = {}


def _scene(n):
    if n not in _scenes:
        v = 16384 if n >= 257 else 1000
        empties = n % 2 == 1
        clusters = {257: (12, 51), 1329: (51, 257)}.get(n, (5,))
        _scenes[n] = Scene(n, v, seed=1000 + n, empties=empties, clusters=clusters)
    return _scenes[n]


@pytest.fixture(scope="module")
def scored(ctx):
    """n -> (scene, fp64 S, nnz, device S); computed once per module"""
    cache = {}

    def get(n):
        if n not in cache:
            sc = _scene(n)
            _upload(ctx, sc.images)
            ctx.set_vocabulary(sc.words)
            s, nnz = sc.reference(ctx)
            _, _, m = ctx.retrieve_pairs(sc.order, 5, score_matrix=True)
            cache[n] = (sc, s, nnz, m)
        return cache[n]
    return get


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 257, 1329])
def test_scores_across_tiles(ctx, scored, n):
    sc, s, nnz, m1 = scored(n)
    _upload(ctx, sc.images)
    ctx.set_vocabulary(sc.words)
    _, _, m2 = ctx.retrieve_pairs(sc.order, 5, score_matrix=True)
    assert np.array_equal(_bits(m1), _bits(m2))                       # two calls, the same bits
    assert np.array_equal(_bits(m1), _bits(m1.T))                     # the mirrored stores
    off = ~np.eye(n, dtype=bool)
    bound = ref.score_bound(nnz[:, None], nnz[None, :])
    err = np.abs(m1.astype(np.float64) - s)
    assert np.all(err[off] <= bound[off]), float((err[off] / bound[off]).max())
    assert np.all(np.diag(m1) == 0)
    # the planted specials: a zero vector has no candidates, every image of a cluster exactly size - 1
    for p, role in enumerate(sc.roles):
        cnt = int((m1[p] > 0).sum())
        if role in ("empty", "idf0") or (role == "zero" and n % 2 == 0):
            assert cnt == 0, (p, role)
        if isinstance(role, tuple):
            assert cnt == sc.roles.count(role) - 1, (p, role)
    assert (s[off] > 0).mean() > 0.02
    # the same images under permuted ids: pairs move to other tiles and across the diagonal, the bits do not change
    sigma = np.random.default_rng(n).permutation(n)
    _upload(ctx, sc.images, idmap=sigma)
    _, _, m3 = ctx.retrieve_pairs(sc.order, 5, score_matrix=True)
    assert np.array_equal(_bits(m3[np.ix_(sigma, sigma)]), _bits(m1))


def _check_selection(pairs, scores, m, s, nnz, order, k):
    got = [tuple(p) for p in pairs.tolist()]
    assert got == sorted(set(got)) and all(a > b for a, b in got)       # brute mode's orientation and order
    assert got == ref.select_fast(m, order, k)                          # the rule, exactly, on the device scores
    pos = {i: p for p, i in enumerate(order)}
    ia = np.array([pos[a] for a, _ in got], np.int64)
    ib = np.array([pos[b] for _, b in got], np.int64)
    assert np.array_equal(_bits(np.asarray(scores, np.float32)), _bits(m[ia, ib]))
    # the fp64 selection, on every row not within 2 bound of a tie at the K-th place
    gotset = set(got)
    top = ref.select_rows(s, order, k)
    checked = 0
    for a in range(len(order)):
        row = s[a].copy()
        row[a] = 0
        srt = np.sort(row[row > 0])[::-1]
        b2 = 2 * ref.score_bound(nnz[a], nnz).max()
        if len(srt) > k and srt[k - 1] - srt[k] <= b2:
            continue
        for j in top[a].tolist():
            assert (max(order[a], order[j]), min(order[a], order[j])) in gotset, (a, j, k)
        checked += 1
    return checked


TOPK_K = [1, 50, 255, 256, 257, 511, 512, 513, 1024]


@pytest.mark.parametrize("n", [257, 1329])
@pytest.mark.parametrize("k", TOPK_K)
def test_topk_loop_and_sort_edges(ctx, scored, n, k):
    sc, s, nnz, m1 = scored(n)
    _upload(ctx, sc.images)
    ctx.set_vocabulary(sc.words)
    pairs, scores, m = ctx.retrieve_pairs(sc.order, k, score_matrix=True)
    assert np.array_equal(_bits(m), _bits(m1))
    checked = _check_selection(pairs, scores, m, s, nnz, sc.order, k)
    assert checked >= n // 2
    if k >= n - 1:   # every positive pair
        want = sorted((max(a, b), min(a, b)) for a in range(n) for b in range(a) if m[a, b] > 0)
        assert [tuple(p) for p in pairs.tolist()] == want


def test_topk_cases_cover_every_candidate_count(scored):
    # across the cases above, some image has 0, < K, = K and > K candidates (s > 0, not itself)
    seen = set()
    for n in (257, 1329):
        cnt = (scored(n)[3] > 0).sum(1)
        for k in TOPK_K:
            seen |= {"0" if c == 0 else "<K" if c < k else "=K" if c == k else ">K" for c in cnt.tolist()}
    assert seen == {"0", "<K", "=K", ">K"}
    assert ((scored(1329)[3] > 0).sum(1) > 512).any()   # K = 1024 sorts 1024 keys


@pytest.mark.parametrize("k", [1, 50, 299, 300, 512])
def test_hundreds_of_identical_images_tie_to_the_lowest_ids(ctx, k):
    rng = np.random.default_rng(77)
    n, nd, v = 700, 300, 2000
    words = rng.integers(0, 256, size=(v, 128)).astype(np.uint8)
    dup_idx = np.concatenate([np.arange(20), rng.choice(np.arange(20), size=40), [500, 501]])   # 2 words shared with others
    dup = words[dup_idx]
    ids = np.sort(rng.choice(np.arange(3000), size=n, replace=False))   # ids above 255: the radix select needs their two low bytes
    dups = set(rng.choice(ids, size=nd, replace=False).tolist())
    images = {}
    for i in ids.tolist():
        if i in dups:
            images[i] = dup.copy()
        else:
            idx = rng.choice(np.arange(20, v), size=int(rng.integers(3, 30)))
            images[i] = words[idx]
    _upload(ctx, images)
    ctx.set_vocabulary(words)
    order = ids.tolist()
    pairs, scores, m = ctx.retrieve_pairs(order, k, score_matrix=True)
    got = [tuple(p) for p in pairs.tolist()]
    assert got == ref.select_fast(m, order, k)
    d = sorted(dups)
    pos = {i: p for p, i in enumerate(order)}
    dp = np.array([pos[i] for i in d])
    # every pair of twins has the same bits, above any score with another image
    tw = m[np.ix_(dp, dp)][~np.eye(nd, dtype=bool)]
    assert np.all(_bits(tw) == _bits(tw[:1]))
    other = np.setdiff1d(np.arange(n), dp)
    assert m[np.ix_(dp, other)].max() < tw[0]
    assert (m[np.ix_(dp, other)] > 0).any()
    # twin d_y takes the K lowest of its twins: the pair of d_x < d_y is selected iff x < K
    want = {(d[y], d[x]) for y in range(nd) for x in range(y) if x < k}
    assert {p for p in got if p[0] in dups and p[1] in dups} == want


def test_ten_thousand_images(ctx):
    n, v, k = 10000, 256, 1024   # MSFM_MAX_IMAGES
    rng = np.random.default_rng(99)
    words = rng.integers(0, 256, size=(v, 128)).astype(np.uint8)
    expect, images = [], {}
    for p in range(n):
        idx = rng.integers(0, v, size=int(rng.integers(0, 5)) if p % 97 else 0)
        expect.append(idx)
        images[p] = words[idx] if p % 2 else words[idx].astype(np.float32) / np.float32(255.0)
    _upload(ctx, images)
    ctx.set_vocabulary(words)
    for p in range(0, n, 37):
        assert np.array_equal(ctx.image_words(p), expect[p]), p
    order = list(range(n))
    pairs, scores, m = ctx.retrieve_pairs(order, k, score_matrix=True)   # 400 MB on the host
    rows = np.unique(np.concatenate([[0, 1, 63, 64, 4999, 9935, 9936, 9998, 9999], rng.choice(n, size=60, replace=False)]))
    s, nnz = ref.scores_from_words(expect, v, rows=rows)
    mr = m[rows]
    assert np.array_equal(_bits(mr), _bits(m[:, rows].T))
    bound = ref.score_bound(nnz[rows][:, None], nnz[None, :])
    off = np.ones(mr.shape, bool)
    off[np.arange(len(rows)), rows] = False
    err = np.abs(mr.astype(np.float64) - s)
    assert np.all(err[off] <= bound[off]), float((err[off] / bound[off]).max())
    got = set(map(tuple, pairs.tolist()))
    assert np.array_equal(_bits(scores), _bits(m[pairs[:, 0], pairs[:, 1]]))
    dev = ref.select_rows(mr, order, k, rows=rows)
    fp = ref.select_rows(s, order, k, rows=rows)
    checked = 0
    for r, a in enumerate(rows.tolist()):
        for j in dev[r].tolist():
            assert (max(a, j), min(a, j)) in got
        srt = np.sort(s[r][off[r] & (s[r] > 0)])[::-1]
        if len(srt) > k and srt[k - 1] - srt[k] <= 2 * bound[r].max():
            continue
        assert set(dev[r].tolist()) == set(fp[r].tolist()), a
        checked += 1
    assert checked >= len(rows) // 2
    del m


@pytest.mark.parametrize("v", [16385, 24576, 32769, 65536])
def test_assignment_beyond_two_passes(ctx, v):
    rng = np.random.default_rng(v)
    words = rng.integers(0, 256, size=(v, 128)).astype(np.uint8)
    # duplicates straddling the pass boundaries: the lower word wins (not at V = 16385, whose third pass holds word 16384 alone)
    dups = [lo for lo in (8191, 16383, 57343) if lo + 1 < v - 1]
    for lo in dups:
        words[lo + 1] = words[lo]
    if v == 65536:
        words[65535] = words[100]
    marks = [0, 100, 8191, 8192, 8193, 16383, 16384, 24575, 32767, 32768, 57343, 57344, 65535, v - 1]
    marks += [int(x) for x in rng.integers(0, v, size=40)]
    planted = np.array([m_ for m_ in marks if m_ < v])

    def near(idx, jitter):
        x = words[idx].astype(np.int64) + rng.integers(-jitter, jitter + 1, size=(len(idx), 128))
        return np.clip(x, 0, 255).astype(np.uint8)

    def mixed(r):
        idx = rng.choice(planted, size=r)
        x = near(idx, 2)
        x[::3] = rng.integers(0, 256, size=x[::3].shape)   # some rows far from every word
        return x

    images = {k_: mixed(r) for k_, r in enumerate([255, 256, 257])}
    images[3] = near(planted, 1).astype(np.float32) / np.float32(255.0)
    images[4] = np.zeros((0, 128), np.uint8)
    uniq = mixed(1024)
    tile = rng.integers(0, 1024, size=65537)
    tile[:1024] = np.arange(1024)
    images[5] = uniq[tile]                                 # 65 537 rows over 1024 distinct ones
    _upload(ctx, images)
    ctx.set_vocabulary(words)
    for i, x in images.items():
        if i == 5:
            want = ref.assign(ref.quantize(uniq), words)[tile]
        else:
            want = ref.assign(ref.quantize(x), words)
        got = ctx.image_words(i)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (i, v, np.flatnonzero(got != want)[:5])
    # nearest words in every pass, and the lower of two identical words
    allw = np.concatenate([ctx.image_words(i) for i in images])
    assert set((allw // 8192).tolist()) == set(range((v + 8191) // 8192))
    for lo in dups:
        assert lo in allw and lo + 1 not in allw
    if v == 65536:
        assert 100 in allw and 65535 not in allw


@pytest.mark.parametrize("v,rows,want_v", [(1024, 16384, 1024), (2048, 12000, 1500)])
def test_training_at_a_larger_shape(ctx, v, rows, want_v):
    rng = np.random.default_rng(v)
    protos = rng.integers(0, 256, size=(3000, 128))
    images = {}
    for i in range(230):
        r = 0 if i % 17 == 5 else int(rng.integers(1, 400))
        x = np.clip(protos[rng.integers(0, 3000, size=r)] + rng.integers(-8, 9, size=(r, 128)), 0, 255).astype(np.uint8)
        images[i] = x.astype(np.float32) / np.float32(255.0) if i % 5 == 2 else x
    ids = rng.permutation(list(images)).tolist()
    _upload(ctx, images)
    total = sum(len(x) for x in images.values())
    step, count = ref.sample_plan(total, rows)
    assert step > 1 and ref.vocab_size(v, count) == want_v
    want, _ = ref.train(images, ids, num_words=v, iters=8, max_rows=rows)
    got = ctx.train_vocabulary(ids, num_words=v, train_iters=8, train_rows=rows)
    assert got.shape == want.shape == (want_v, 128)
    assert np.array_equal(got, want)


ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
YAML = """%YAML:1.0
database_path : "{db}"
SIFTmatch.match_type : {mt}
SIFTmatch.num_nearest_images : {k}
SIFTmatch.vocab_num_words : {v}
SIFTmatch.vocab_train_iters : 8
"""


def test_executable_beyond_one_score_tile(built_lib, ctx, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "ComputeMatches")
    n, k, v = 136, 110, 256
    images, _ = ref.covis_scene(n, window=40, stride=8, per_proto=1, fresh=20, jitter=3, seed=13, as_float=True)
    descs = [np.ascontiguousarray(images[i], np.float32) for i in range(n)]
    kps = [synth.keypoints(len(d), seed=300 + i) for i, d in enumerate(descs)]
    env = dict(os.environ, MSFM_GEOMETRIC_VERIFICATION="0", MSFM_TRACE_TRANSACTIONS="1")
    res = {}
    for name, mt in (("vocab", 2), ("brute", 1)):
        path = str(tmp_path / (name + ".db"))
        database.write_synthetic_database(path, descs, kps)
        cfg = tmp_path / (name + ".yaml")
        cfg.write_text(YAML.format(db=path, mt=mt, k=k, v=v))
        r = subprocess.run([exe, str(cfg)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = database.Database(path)
        rows = d.db.execute("SELECT pair_id, rows, cols, data FROM matches ORDER BY pair_id").fetchall()
        d.Close()
        res[name] = (r, rows)
    # the library's retrieval on the same images
    ctx.clear_images()
    for i, x in enumerate(descs):
        ctx.upload_image(i, x)
    ids = list(range(n))
    ctx.train_vocabulary(ids, num_words=v, train_iters=8)
    pairs, _ = ctx.retrieve_pairs(ids, k)
    pairs = [tuple(p) for p in pairs.tolist()]
    r, rows = res["vocab"]
    assert sorted(x[0] for x in rows) == sorted(database.ImagePairToPairId(i, j) for i, j in pairs)
    seen = [tuple(map(int, x)) for x in re.findall(r"Compute Matches (\d+) - (\d+) \.\.\. \n", r.stdout)]
    assert seen == pairs
    # one transaction per group, the groups of msfm_ret_group_ends (rows longer than 100 pairs split)
    ends = ref.group_ends(pairs, 100)
    sizes = [b - a for a, b in zip([0] + ends[:-1], ends)]
    assert [int(x) for x in re.findall(r"\[msfm txn\] (\d+)", r.stderr)] == sizes
    assert sizes.count(100) >= 2 and max(sum(1 for p in pairs if p[0] == i) for i in range(n)) > 100
    # rows of mode 2 equal mode 1's rows for the same pair
    brute = {x[0]: x for x in res["brute"][1]}
    shared = [x for x in rows if x[0] in brute]
    assert len(shared) >= 100 and sum(x[1] > 0 for x in shared) >= 50
    for x in shared:
        assert x == brute[x[0]]
