"""numpy reference of vocabulary retrieval (matching mode 2, include/msfm_match.h "vocabulary retrieval").

Everything up to the scores is integer arithmetic: the nearest word uses an fp64 matmul, exact because every product and partial sum is
an integer below 2^53, and np.argmin keeps the lower word on a tie.  The scores are the fp64 definition.  Also a seeded co-visibility
scene whose true overlaps are known.
"""
import numpy as np


def quantize(x):
    """q (int64, n x 128) of one image: the values if all are integers in 0..255, rint(255 x) (fp32 multiply, half to even) if all
    lie in [0, 1]; ValueError otherwise."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x.astype(np.int64)
    x = x.astype(np.float32)
    if x.size == 0 or (np.all(x == np.floor(x)) and np.all(x >= 0) and np.all(x <= 255)):
        return x.astype(np.int64)
    if np.all(x >= 0) and np.all(x <= 1):
        return np.rint(x * np.float32(255.0)).astype(np.int64)
    raise ValueError("values neither integers in [0, 255] nor in [0, 1]")


def assign(q, words, block_bytes=256 << 20):
    """the nearest word of every row: argmin_w |c'_w|^2 - 2 q'.c'_w, the lower w on a tie.  Rows go in chunks whose fp64 key block
    stays within `block_bytes`; every row's key is the same whatever the chunk, so the result does not depend on it."""
    q = np.asarray(q, np.int64).reshape(-1, 128)
    if len(q) == 0:
        return np.zeros(0, np.int64)
    c = np.asarray(words, np.int64).reshape(-1, 128) - 128
    cn = (c * c).sum(1)[None, :].astype(np.float64)
    ct = c.T.astype(np.float64)
    step = max(1, int(block_bytes) // (8 * len(c)))
    out = np.empty(len(q), np.int64)
    for r0 in range(0, len(q), step):
        qq = (q[r0:r0 + step] - 128).astype(np.float64)
        out[r0:r0 + step] = np.argmin(cn - 2.0 * (qq @ ct), axis=1)
    return out


def sample_plan(rows, max_rows):
    s = max(1, rows // max_rows) if max_rows > 0 else 1
    n = min(max_rows, (rows + s - 1) // s) if rows > 0 else 0
    return s, n


def vocab_size(num_words, sample_rows):
    return min(num_words, max(1, sample_rows // 8))


def initial_rows(vocab, sample_rows):
    return [(k * sample_rows) // vocab for k in range(vocab)]


def centroid(total, cnt):
    return (2 * total + cnt) // (2 * cnt)


def concat(images, ids):
    order = sorted(ids)
    qs = [quantize(images[i]) for i in order]
    return order, (np.concatenate(qs) if qs else np.zeros((0, 128), np.int64)), [len(q) for q in qs]


def train(images, ids, num_words=16384, iters=8, max_rows=None):
    """integer k-means on the sample -> (words V' x 128 uint8, iterations run)"""
    if max_rows is None:
        max_rows = min(64 * num_words, 1 << 24)
    _, q, _ = concat(images, ids)
    s, ms = sample_plan(len(q), max_rows)
    smp = q[0:s * ms:s][:ms]
    vp = vocab_size(num_words, ms)
    c = smp[initial_rows(vp, ms)].copy()
    done = 0
    for _ in range(iters):
        w = assign(smp, c)
        done += 1
        sums = np.zeros((vp, 128), np.int64)
        np.add.at(sums, w, smp)
        cnt = np.bincount(w, minlength=vp).astype(np.int64)
        new = c.copy()
        has = cnt > 0
        new[has] = centroid(sums[has], cnt[has][:, None])
        changed = not np.array_equal(new, c)
        c = new
        if not changed:
            break
    return c.astype(np.uint8), done


def histograms(images, ids, words):
    """c_iw per image, in ascending id order"""
    order = sorted(ids)
    v = len(words)
    h = np.zeros((len(order), v), np.int64)
    for k, i in enumerate(order):
        q = quantize(images[i])
        if len(q):
            h[k] = np.bincount(assign(q, words), minlength=v)
    return order, h


def scores(images, ids, words):
    """-> (ids ascending, fp64 S (0 on the diagonal), nnz per image)"""
    order, h = histograms(images, ids, words)
    n = len(order)
    nw = (h > 0).sum(0)
    idf = np.where(nw > 0, np.log(n / np.maximum(nw, 1)), 0.0)
    v = h * idf[None, :]
    nrm = np.sqrt((v * v).sum(1))
    a = np.where(nrm[:, None] > 0, v / np.where(nrm > 0, nrm, 1)[:, None], 0.0)
    s = a @ a.T
    np.fill_diagonal(s, 0.0)
    return order, s, (h > 0).sum(1)


def tfidf(h):
    """the fp64 unit tf-idf vectors of the histograms h (n x V, images in ascending id order); 0 for an image whose vector is 0"""
    h = np.asarray(h)
    n = len(h)
    nw = (h > 0).sum(0)
    idf = np.where(nw > 0, np.log(n / np.maximum(nw, 1)), 0.0)
    v = h * idf[None, :]
    nrm = np.sqrt((v * v).sum(1))
    return np.where(nrm[:, None] > 0, v / np.where(nrm > 0, nrm, 1)[:, None], 0.0)


def histograms_from_words(word_lists, v):
    """c_iw from the nearest word of every row of every image (a list of int arrays, ascending id order)"""
    h = np.zeros((len(word_lists), v), np.int64)
    for k, w in enumerate(word_lists):
        if len(w):
            h[k] = np.bincount(np.asarray(w, np.int64), minlength=v)
    return h


def scores_from_words(word_lists, v, rows=None):
    """fp64 S from given per-image words -> (S, nnz per image).  rows=None: the full n x n S (0 on the diagonal), as `scores`;
    otherwise the rows `rows` of it only, a[rows] @ a.T (len(rows) x n, 0 at (r, rows[r]))."""
    h = histograms_from_words(word_lists, v)
    a = tfidf(h)
    nnz = (h > 0).sum(1)
    if rows is None:
        s = a @ a.T
        np.fill_diagonal(s, 0.0)
        return s, nnz
    rows = np.asarray(rows, np.int64)
    s = a[rows] @ a.T
    s[np.arange(len(rows)), rows] = 0.0
    return s, nnz


def select_rows(s, ids, k, rows=None):
    """`topk` of every row of a score matrix, vectorised: a list of arrays of positions.  s is n x n (rows and columns in the order
    of ids), or len(rows) x n for the rows `rows` of it."""
    s = np.asarray(s)
    n = len(ids)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    ids = np.asarray(ids, np.int64)
    cand = s > 0
    cand[np.arange(len(rows)), rows] = False
    sf = s.astype(np.float64)
    order = np.lexsort((np.broadcast_to(ids, s.shape), -np.where(cand, sf, -np.inf)), axis=1)
    cnt = cand.sum(1)
    return [order[r, :min(k, int(cnt[r]))] for r in range(len(rows))]


def select_fast(s, ids, k):
    """`select` through `select_rows`: the same pairs"""
    out = set()
    for i, top in enumerate(select_rows(s, ids, k)):
        for j in top.tolist():
            out.add((max(ids[i], ids[j]), min(ids[i], ids[j])))
    return sorted(out)


def group_ends(pairs, per_group):
    """msfm_ret_group_ends: a group ends after every `per_group` pairs of a row and at the end of every row"""
    ends, in_group = [], 0
    for t in range(len(pairs)):
        in_group += 1
        if in_group == per_group or t + 1 == len(pairs) or pairs[t + 1][0] != pairs[t][0]:
            ends.append(t + 1)
            in_group = 0
    return ends


def score_bound(nnz_i, nnz_j):
    """the documented bound of |s_dev - s|: (min(nnz_i, nnz_j) + 4) 2^-23"""
    return (np.minimum(nnz_i, nnz_j) + 4) * 2.0 ** -23


def topk(s_row, ids, self_pos, k):
    """positions of the first k images j != self with s > 0, highest first, the lower id on equal scores"""
    cand = [j for j in range(len(ids)) if j != self_pos and s_row[j] > 0]
    cand.sort(key=lambda j: (-float(s_row[j]), ids[j]))
    return cand[:k]


def select(s, ids, k):
    """the union of the selections as (max, min) pairs, by first then second id"""
    out = set()
    for i in range(len(ids)):
        for j in topk(s[i], ids, i, k):
            out.add((max(ids[i], ids[j]), min(ids[i], ids[j])))
    return sorted(out)


def covis_scene(n_images, window=8, stride=2, per_proto=40, fresh=60, n_proto=None, jitter=6, seed=0, as_float=False):
    """A planted co-visibility scene: image i observes the prototypes [stride i, stride i + window) -- per_proto jittered rows each --
    plus `fresh` rows nobody else sees.  -> (images {id: rows}, overlap(i, j) = shared fraction of the window)."""
    rng = np.random.default_rng(seed)
    if n_proto is None:
        n_proto = stride * (n_images - 1) + window
    protos = rng.integers(0, 256, size=(n_proto, 128))
    images = {}
    for i in range(n_images):
        rows = []
        for p in range(stride * i, stride * i + window):
            rows.append(np.clip(protos[p][None, :] + rng.integers(-jitter, jitter + 1, size=(per_proto, 128)), 0, 255))
        rows.append(rng.integers(0, 256, size=(fresh, 128)))
        x = np.concatenate(rows).astype(np.uint8)
        rng.shuffle(x)
        images[i] = (x.astype(np.float32) / np.float32(255.0)) if as_float else x

    def overlap(i, j):
        return max(0, window - stride * abs(i - j)) / window

    return images, overlap
