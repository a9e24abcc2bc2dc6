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


def assign(q, words):
    """the nearest word of every row: argmin_w |c'_w|^2 - 2 q'.c'_w, the lower w on a tie"""
    q = np.asarray(q, np.int64).reshape(-1, 128)
    if len(q) == 0:
        return np.zeros(0, np.int64)
    c = np.asarray(words, np.int64).reshape(-1, 128) - 128
    qq = (q - 128).astype(np.float64)
    key = (c * c).sum(1)[None, :].astype(np.float64) - 2.0 * (qq @ c.T.astype(np.float64))
    return np.argmin(key, axis=1)


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
