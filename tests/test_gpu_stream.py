"""The streaming form of the C ABI (msfm_match_pairs_begin / _next): one device sub-batch per call, nothing accumulates in the
library -- the reference streams by construction, one transaction per <= 100 pairs (src/Feature/FeatureMatching.cpp:13, 70-72,
118-139).  The chunks, concatenated, must be the lists msfm_match_pairs returns, bit for bit, under every cut."""
import numpy as np
import pytest

from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def collect(ctx, pairs, **kw):
    offs = [np.zeros(1, np.int64)]
    qt, d, sens = [], [], []
    nxt = 0
    chunks = 0
    for ch in ctx.match_pairs_stream(pairs, **kw):
        assert ch["first"] == nxt and ch["n_pairs"] > 0      # in pair order, contiguous
        assert ch["offsets"][0] == 0 and len(ch["offsets"]) == ch["n_pairs"] + 1 and ch["offsets"][-1] == len(ch["qt"]) == len(ch["dist"])
        offs.append(offs[-1][-1] + ch["offsets"][1:])
        qt.append(ch["qt"])
        d.append(ch["dist"])
        sens.append(ch["sensitive"])
        nxt += ch["n_pairs"]
        chunks += 1
    assert nxt == len(pairs)
    return np.concatenate(offs), np.concatenate(qt) if qt else np.zeros((0, 2), np.int32), np.concatenate(d) if d else np.zeros(0, np.float32), \
        np.concatenate(sens) if sens else np.zeros(0, np.int32), chunks


@pytest.mark.parametrize("kind", ["rootsift", "u8"])
def test_stream_equals_one_call_under_forced_cuts(kind):
    n_img = 12
    if kind == "rootsift":
        imgs = synth.rootsift_images(n_img, [1500, 700, 2100, 64, 900, 1300, 0, 1800, 1000, 400, 1600, 1200], seed=77, n_proto=4000)
        kw = {}
    else:
        imgs = synth.u8_images(n_img, [1500, 700, 2100, 64, 900, 1300, 1, 1800, 1000, 400, 1600, 1200], seed=78, dup_frac=0.2, as_float=False)
        kw = {"max_distance": 1e9}
    pairs = synth.all_pairs(n_img)
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ref = ctx.match_pairs(pairs, **kw)
        cert = ctx.order_certificate(len(pairs))
        for limit in (0, 7, 1):
            ctx.set_limits(max_pairs_per_batch=limit)
            offs, qt, d, sens, chunks = collect(ctx, pairs, **kw)
            assert np.array_equal(offs, ref[0]) and np.array_equal(qt, ref[1]) and np.array_equal(bits(d), bits(ref[2]))
            assert np.array_equal(sens, cert)
            if limit:
                assert chunks == -(-len(pairs) // limit)
        ctx.set_limits()
        # a series left open: the store must not change under it; the next matching call abandons it
        ctx.set_limits(max_pairs_per_batch=7)
        it = ctx.match_pairs_stream(pairs, **kw)
        next(it)
        with pytest.raises(_lib.MsfmError) as err:
            ctx.upload_image(0, imgs[0])
        assert err.value.code == _lib.E_STATE
        with pytest.raises(_lib.MsfmError):
            ctx.clear_images()
        ctx.set_limits()
        again = ctx.match_pairs(pairs, **kw)
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
        with pytest.raises(_lib.MsfmError):
            next(it)          # its series is gone (state error, not stale data)
        # an empty pair list: no chunk
        assert list(ctx.match_pairs_stream(np.zeros((0, 2), np.int32))) == []


def test_stream_with_verification_equals_the_verified_call():
    imgs = synth.rootsift_images(5, [1200, 1100, 900, 1000, 1300], seed=79, n_proto=2500)
    pairs = synth.all_pairs(5)
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
            ctx.upload_keypoints(i, synth.keypoints(len(im), seed=100 + i))
        ref = ctx.match_pairs_verified(pairs)
        ctx.set_limits(max_pairs_per_batch=3)
        offs, qt, d, _, chunks = collect(ctx, pairs, verified=True)
        assert chunks == 4
        assert np.array_equal(offs, ref[0]) and np.array_equal(qt, ref[1]) and np.array_equal(bits(d), bits(ref[2]))


def test_stream_device_pointers_hold_the_same_lists():
    imgs = synth.u8_images(4, [2000, 1500, 1800, 900], seed=80, dup_frac=0.3, as_float=False)
    pairs = synth.all_pairs(4)
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ctx.set_limits(max_pairs_per_batch=2)
        seen = 0
        for ch in ctx.match_pairs_stream(pairs, max_distance=1e9, copy=False):
            m = len(ch["qt"])
            if m == 0:
                continue
            assert np.array_equal(ctx.read_device(ch["d_qt"], (m, 2), np.int32), ch["qt"])
            assert np.array_equal(bits(ctx.read_device(ch["d_dist"], (m,), np.float32)), bits(ch["dist"]))
            seen += m
        assert seen > 100


def test_knn2_pair_and_an_early_exit_both_end_an_open_series():
    """(1) msfm_knn2_pair in the middle of a series abandons it like any other matching call (it ran on scratch set 0 with the
    series' sub-batches in flight and the next _next handed out foreign offsets): the following _next is a state error, the kNN lists are
    the ones a fresh context gives.  (2) A consumer that breaks out of the generator leaves no series open: msfm_match_pairs_end
    unlocks the store, uploads work again, and a later series still equals the one-call result."""
    imgs = synth.u8_images(8, [900, 1400, 700, 1100, 1300, 600, 1000, 1200], seed=81, dup_frac=0.2, as_float=False)
    pairs = synth.all_pairs(8)
    kw = {"max_distance": 1e9}
    with _lib.Context(0) as ref_ctx:
        for i, im in enumerate(imgs):
            ref_ctx.upload_image(i, im)
        knn_ref = ref_ctx.knn2_pair(3, 1)
        ref = ref_ctx.match_pairs(pairs, **kw)
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ctx.set_limits(max_pairs_per_batch=3)
        it = ctx.match_pairs_stream(pairs, **kw)
        first = next(it)
        assert first["n_pairs"] == 3
        knn = ctx.knn2_pair(3, 1)                       # sub-batches 2 and 3 of the series are in flight here
        for a, b in zip(knn, knn_ref):
            assert np.array_equal(bits(a), bits(b))
        with pytest.raises(_lib.MsfmError) as err:
            next(it)
        assert err.value.code == _lib.E_STATE
        ctx.upload_image(0, imgs[0])                    # the store is unlocked
        # (2) early exit
        for k, ch in enumerate(ctx.match_pairs_stream(pairs, **kw)):
            if k == 1:
                break
        ctx.upload_image(1, imgs[1])                    # no E_STATE: the generator's finally ended the series
        assert ctx._L.msfm_match_pairs_end(ctx._h) == 0   # nothing open: a no-op
        it = ctx.match_pairs_stream(pairs, **kw)
        next(it)
        it.close()                                      # GeneratorExit takes the same path
        ctx.clear_images()
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        offs, qt, d, _, chunks = collect(ctx, pairs, **kw)
        assert chunks == -(-len(pairs) // 3)
        assert np.array_equal(offs, ref[0]) and np.array_equal(qt, ref[1]) and np.array_equal(bits(d), bits(ref[2]))


@pytest.fixture(scope="module")
def eight_u8():
    """The images of test_knn2_pair_and_an_early_exit_both_end_an_open_series and their one-call lists."""
    imgs = synth.u8_images(8, [900, 1400, 700, 1100, 1300, 600, 1000, 1200], seed=81, dup_frac=0.2, as_float=False)
    pairs = synth.all_pairs(8)
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ref = ctx.match_pairs(pairs, max_distance=1e9)
    return imgs, pairs, ref


def rest_of(it, first, n_pairs):
    """The chunks of the generator `it` behind `first`, joined to it like collect() joins them."""
    offs, qt, d, nxt = [np.zeros(1, np.int64)], [], [], 0
    for ch in [first] + list(it):
        assert ch["first"] == nxt and ch["n_pairs"] > 0
        offs.append(offs[-1][-1] + ch["offsets"][1:])
        qt.append(ch["qt"])
        d.append(ch["dist"])
        nxt += ch["n_pairs"]
    assert nxt == n_pairs
    return np.concatenate(offs), np.concatenate(qt), np.concatenate(d)


@pytest.mark.parametrize("how", ["close", "collect"])
def test_a_stale_generator_does_not_end_a_newer_series(eight_u8, how):
    """A generator whose series a newer one on the same context has superseded is closed, or dropped and collected, while the newer
    series is under way: its `finally` must not call msfm_match_pairs_end, which knows no owner -- the newer series'
    next chunk used to fail with E_STATE in mid-job.  Its own next() is a state error, not a chunk of the newer series."""
    import gc
    imgs, pairs, ref = eight_u8
    kw = {"max_distance": 1e9}
    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ctx.set_limits(max_pairs_per_batch=3)          # ten chunks, two sub-batches in flight behind each
        a0 = ctx.match_pairs_stream(pairs, **kw)
        assert next(a0)["n_pairs"] == 3
        a = ctx.match_pairs_stream(pairs, **kw)
        assert next(a)["n_pairs"] == 3
        b = ctx.match_pairs_stream(pairs, **kw)
        first = next(b)
        with pytest.raises(_lib.MsfmError) as err:      # a0 is suspended at its first chunk; a and b came after it
            next(a0)
        assert err.value.code == _lib.E_STATE
        if how == "close":
            a.close()
        else:
            del a
            gc.collect()
        offs, qt, d = rest_of(b, first, len(pairs))     # at the parent of this change: E_STATE at b's second chunk
        assert np.array_equal(offs, ref[0]) and np.array_equal(qt, ref[1]) and np.array_equal(bits(d), bits(ref[2]))
        ctx.upload_image(0, imgs[0])                    # b ran to its end: the store is unlocked


def test_a_series_that_fails_is_closed_and_nothing_of_it_is_left(eight_u8):
    """The lifecycle rows of DESIGN.md 4.3 for a streaming call that fails without a device error.  An image that was never uploaded
    is reported by the msfm_match_pairs_next that first builds its pair (msfm_match_pairs_begin looks at no image), an image id out of
    range by msfm_match_pairs_begin itself.  After either: _next is E_STATE, _end is a no-op, the store is unlocked, and the blocking
    call's lists from before are gone -- msfm_match_pairs_begin had started, and a matching call that starts gives up what the call
    before it handed out."""
    imgs, pairs, ref = eight_u8
    L = _lib.load()
    prm = _lib.MatchParams(0.8, 1, 1e9)
    ch = _lib.Chunk()

    def begin(ctx, plist):
        plist = np.ascontiguousarray(plist, np.int32)
        return L.msfm_match_pairs_begin(ctx._h, _lib._ip(plist), len(plist), _lib.C.byref(prm), 0, None)

    def closed_and_empty(ctx):
        assert L.msfm_match_pairs_next(ctx._h, _lib.C.byref(ch)) == _lib.E_STATE
        assert L.msfm_match_pairs_end(ctx._h) == _lib.OK
        ctx.upload_image(7, imgs[7])
        assert L.msfm_fetch_matches(ctx._h, None, None) == _lib.E_STATE

    with _lib.Context(0) as ctx:
        for i, im in enumerate(imgs):
            ctx.upload_image(i, im)
        ctx.set_limits(max_pairs_per_batch=3)
        for bad in ([[0, 1], [2, 3], [4, 9], [5, 6]], [[0, 1], [2, 3 * _lib.MAX_IMAGES]]):
            again = ctx.match_pairs(pairs, max_distance=1e9)
            assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
            assert L.msfm_fetch_matches(ctx._h, None, None) == _lib.OK
            rc = begin(ctx, bad)
            if bad[-1][1] > 2 * _lib.MAX_IMAGES:       # (the slots go on to 2 * MAX_IMAGES + 1)
                assert rc == _lib.E_INVALID             # image id out of range: found before the first launch
            else:
                assert rc == _lib.OK                    # image 9 was never uploaded: the first sub-batch finds out
                assert L.msfm_match_pairs_next(ctx._h, _lib.C.byref(ch)) == _lib.E_NOIMAGE
            closed_and_empty(ctx)
        # an argument error before the call starts leaves everything as it was: the lists of the call before stay fetchable
        again = ctx.match_pairs(pairs, max_distance=1e9)
        assert L.msfm_match_pairs_begin(ctx._h, None, 3, _lib.C.byref(prm), 0, None) == _lib.E_INVALID
        qt = np.empty((len(ref[1]) + 1, 2), np.int32)
        d = np.empty(len(ref[1]) + 1, np.float32)
        assert L.msfm_fetch_matches(ctx._h, _lib._ip(qt), _lib._fp(d)) == _lib.OK
        assert np.array_equal(qt[:-1], ref[1]) and np.array_equal(bits(d[:-1]), bits(ref[2]))


def test_one_thread_alternates_the_series_of_two_devices():
    """msfm_match_pairs_next selects its context's device: one thread takes the chunks of a series on device 0 and of one
    on device 1 in turn -- every step allocates its scratch and asks for the free memory on its own device -- and both equal the
    one-call lists."""
    if _lib.device_count() < 2:
        pytest.skip("needs two gfx950 devices")
    imgs = synth.u8_images(4, [2000, 1500, 1800, 900], seed=80, dup_frac=0.3, as_float=False)
    pairs = synth.all_pairs(4)
    kw = {"max_distance": 1e9}
    with _lib.Context(0) as c0, _lib.Context(1) as c1:
        for ctx in (c0, c1):
            for i, im in enumerate(imgs):
                ctx.upload_image(i, im)
        ref = c0.match_pairs(pairs, **kw)
        for ctx in (c0, c1):
            ctx.set_limits(max_pairs_per_batch=2)
        its = [c0.match_pairs_stream(pairs, **kw), c1.match_pairs_stream(pairs, **kw)]
        chunks = [[], []]
        while its[0] or its[1]:                         # three chunks of two pairs each, taken in turn
            for k in (0, 1):
                ch = next(its[k], None) if its[k] else None
                if ch is None:
                    its[k] = None
                else:
                    chunks[k].append(ch)
        for k in (0, 1):
            assert len(chunks[k]) == 3
            offs, qt, d = rest_of(chunks[k][1:], chunks[k][0], len(pairs))
            assert np.array_equal(offs, ref[0]) and np.array_equal(qt, ref[1]) and np.array_equal(bits(d), bits(ref[2]))
