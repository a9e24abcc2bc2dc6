"""The hand-out of sweep 1's work items -- equal-cost XCD chunks, per-XCD cursors read one item ahead, workgroups that move on to the
next chunk (msfm_item_chunks, ItemWalk) -- must be invisible in the results: every job below equals the C oracle bit for bit, on
every kernel that walks such a list (integer sweep 1 on byte stores and on the twins of float stores, fp16 sweep 1, both in a
mixed sub-batch), twice in one context (the cursors are cleared per sub-batch).

The jobs are the smallest ones where the hand-out can go wrong: one item (seven empty chunks, 255 workgroups without work), fewer
items than workgroups, item counts that are no multiple of 8, and pairs of 1 x 5400 and 5400 x 1 rows next to 600 x 600 and
5400 x 5400 ones -- an extreme cost ratio, last blocks with 1 and with 16 active waves, chunks of very different lengths, so that
workgroups change chunk.  Small sub-batches split the streamed image into B ranges (assign_partials fills 4 x the CUs), so
`ranges > 1` comes with them."""
import numpy as np
import pytest

from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [5400, 5400, 1, 600, 600, 1300, 513, 40]
JOBS = {
    "mixed sizes": [(2, 0), (0, 2), (3, 4), (4, 3), (0, 1), (5, 6), (6, 7), (7, 5), (3, 5), (1, 3)],
    "fewer items than workgroups": [(3, 4), (7, 6)],
    "one item": [(7, 2)],
}


def b(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def check_vs_oracle(oracle, imgs, pairs, res, **kw):
    offs, qt, d = res
    o_offs, oq, ot, od = oracle.match_pairs(imgs, pairs, nthreads=8, **kw)
    assert np.array_equal(np.asarray(offs), np.asarray(o_offs))
    assert np.array_equal(qt[:, 0], oq) and np.array_equal(qt[:, 1], ot)
    assert np.array_equal(b(d), b(od))
    return int(o_offs[-1])


@pytest.fixture(scope="module")
def float_images():
    return synth.rootsift_images(len(SIZES), SIZES, seed=91, n_proto=1200)


@pytest.fixture(scope="module")
def expected(oracle, float_images):
    """The oracle's lists of every job on the float images, computed once."""
    return {name: oracle.match_pairs(float_images, np.array(p, np.int32), nthreads=8) for name, p in JOBS.items()}


@pytest.mark.parametrize("route", ["twins", "fp16", "mixed"])
def test_float_stores(float_images, expected, oracle, monkeypatch, route):
    monkeypatch.setenv("MSFM_Q8", "2")   # twins for small images too
    imgs = [im.copy() for im in float_images]
    expect = expected
    if route == "mixed":   # one value outside [0, 1]: no twin for image 4, its pairs take the fp16 sweep 1 beside the twins' sweep
        imgs[4][0, int(np.argmin(imgs[4][0]))] = -1e-3
        expect = {name: oracle.match_pairs(imgs, np.array(p, np.int32), nthreads=8) for name, p in JOBS.items()}
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ctx.set_prefilter(2 if route == "fp16" else 1)
        launches = {"i8": 0, "mixed": 0, "pairs": 0}
        for name, p in JOBS.items():
            pairs = np.array(p, np.int32)
            o_offs, oq, ot, od = expect[name]
            for _ in range(2):
                offs, qt, d = ctx.match_pairs(pairs)
                prof = ctx.profile()
                launches["i8"] += prof["sweep1_i8_launches"]
                launches["mixed"] += prof["mixed_route_sub_batches"]
                launches["pairs"] += prof["prefilter_pairs"]
                assert np.array_equal(np.asarray(offs), np.asarray(o_offs)), name
                assert np.array_equal(qt[:, 0], oq) and np.array_equal(qt[:, 1], ot), name
                assert np.array_equal(b(d), b(od)), name
        assert sum(int(e[0][-1]) for e in expect.values()) > 100          # (the jobs do produce matches)
        assert launches["pairs"] == 2 * sum(len(p) for p in JOBS.values())  # every pair went through the sweeps
        assert (launches["i8"] > 0) == (route != "fp16") and (launches["mixed"] > 0) == (route == "mixed")


def test_byte_store(oracle):
    u = synth.u8_images(len(SIZES), SIZES, seed=92, dup_frac=0.2, as_float=False)
    as_float = [im.astype(F32) for im in u]
    kw = {"ratio": 0.8, "cross_check": True, "max_distance": 1e9}
    with _lib.Context(0) as ctx:
        for i, im in enumerate(u):
            ctx.upload_image(i, im)
        matches = 0
        for name, p in JOBS.items():
            pairs = np.array(p, np.int32)
            for _ in range(2):
                res = ctx.match_pairs(pairs, **kw)
                assert ctx.profile()["sweep1_i8_launches"] >= 1, name
                matches += check_vs_oracle(oracle, as_float, pairs, res, **kw)
        assert matches > 100
