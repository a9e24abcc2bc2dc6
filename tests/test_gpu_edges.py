"""Every matching route on rows planted at the decision edges of the reference and at the worst-case roundings of the prefilter
bounds (tests/edge_fixtures.py; tests/test_edge_fixtures.py proves on the CPU that the plants are what they claim).  Each case
compares the match lists with the exact references -- oracle/int_oracle.py for byte values, the C oracle under the same
accumulation order for floats -- for both cross_check values, the knn2 arrays bit for bit where the API exposes them, and
asserts the profile counters that show the route under test was the one taken."""
import numpy as np
import pytest

import edge_fixtures as ef
from monocularsfm_amd import _lib
from oracle import int_oracle as io
from test_gpu_certificate import predicate

pytestmark = pytest.mark.gpu
F32 = np.float32
I8, F16, BRUTE = 1, 2, 0
RATIOS = (0.8, 0.95, float(ef.nextf(0.95, 1)), 1.0, float(ef.nextf(1.0, 2)))


def b(a):
    return np.asarray(a).view(np.int32)


def compare_lists(res, imgs, pairs, ref, what):
    offs, qt, d = res
    for p, (i, j) in enumerate(pairs):
        q, t, dd = ref(imgs[i], imgs[j])
        s, e = int(offs[p]), int(offs[p + 1])
        assert np.array_equal(qt[s:e, 0], q) and np.array_equal(qt[s:e, 1], t), (what, p)
        assert np.array_equal(b(d[s:e]), b(np.asarray(dd, F32))), (what, p)


def compare_knn(ctx, imgs, pairs, ref_knn, what, prefiltered=None):
    for p, (i, j) in enumerate(pairs):
        got = ctx.knn2_pair(int(i), int(j))
        if prefiltered is not None:
            prof = ctx.profile()
            assert prof["prefilter_pairs"] == (1 if prefiltered else 0) and prof["fallback_pairs"] == 0, (what, prof)
        for side, (x, y) in enumerate(((imgs[i], imgs[j]), (imgs[j], imgs[i]))):
            gi, gd0, gd1 = got[side]
            oi0, od0, _, od1 = ref_knn(x, y)
            assert np.array_equal(gi, oi0) and np.array_equal(b(gd0), b(od0)) and np.array_equal(b(gd1), b(od1)), (what, p, side)


def assert_route(prof, mode, ratio, n_pairs, i8_expected=None):
    compact = ratio <= 0.95
    if mode == BRUTE:
        assert prof["prefilter_pairs"] == 0 and prof["dist_kernel_launches"] >= 1, prof
        return
    assert prof["prefilter_pairs"] == n_pairs and prof["fallback_pairs"] == 0, prof
    assert (prof["compacted_pairs"] > 0) == compact, prof
    if i8_expected is not None:
        assert (prof["sweep1_i8_launches"] >= 1) == i8_expected, prof


def upload(ctx, imgs, as_float=False):
    ctx.clear_images()
    for k, x in enumerate(imgs):
        ctx.upload_image(k, x.astype(F32) if as_float else x)


def int_ref(ratio, cc, md):
    return lambda A, B: io.match_pair(A, B, ratio, cc, md)


def c_ref(oracle, ratio, cc, md, order=0):
    return lambda A, B: oracle.match_pair(A, B, ratio, cc, md, order=order)


# ------------------------------------------------------------------------------------------------ 1. byte route at eps = 2
def test_byte_route_parity_gaps_and_lowe_boundaries(gpu_ctx):
    """Integer S gaps 0 / 1 / 2 under all norm parities, the 'window' rows only the parity bits keep alive, and (S0, S1) ON / one
    ulp either side of the Lowe boundary at 0.8 and 0.95: integer cores, fp16 cores and brute force, byte and float uploads."""
    g_imgs, g_pairs, _ = ef.byte_gap_fixture()
    r_imgs, r_pairs, _ = ef.byte_boundary_fixture()
    imgs = g_imgs + r_imgs
    pairs = np.concatenate([g_pairs, r_pairs + len(g_imgs)])
    pairs = np.concatenate([pairs, pairs[:, ::-1]])            # both directions as queries
    P = len(pairs)
    try:
        for as_float in (False, True):
            upload(gpu_ctx, imgs, as_float)
            for mode in (I8, F16, BRUTE):
                gpu_ctx.set_prefilter(mode)
                for ratio in RATIOS:
                    for cc in (True, False):
                        res = gpu_ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=1e9)
                        prof = gpu_ctx.profile()
                        assert_route(prof, mode, ratio, P, i8_expected=(mode == I8 and ratio <= 0.95))
                        assert prof["order_sensitive_rows"] == 0
                        assert gpu_ctx.order_certificate(P).max() == 0       # byte rows: exact under every order
                        compare_lists(res, imgs, pairs, int_ref(ratio, cc, 1e9), (as_float, mode, ratio, cc))
                if not as_float:
                    compare_knn(gpu_ctx, imgs, pairs[:len(pairs) // 2], io.knn2, mode)
    finally:
        gpu_ctx.set_prefilter(True)
        gpu_ctx.clear_images()


def test_byte_distance_cut_boundaries(gpu_ctx):
    """max_distance equal to a planted d0 (as a double), one double either side of it, and doubles that are not floats."""
    imgs, pairs, planted = ef.byte_boundary_fixture(ratios=(0.8,), per_side=2)
    _, d0, _, _ = io.knn2(imgs[0], imgs[1])
    d = float(d0[0])
    cuts = (d, np.nextafter(d, 0), np.nextafter(d, 1e9), d - 2.0 ** -40, d + 2.0 ** -40, 0.7)
    upload(gpu_ctx, imgs)
    try:
        for mode in (I8, BRUTE):
            gpu_ctx.set_prefilter(mode)
            for md in cuts:
                for cc in (True, False):
                    res = gpu_ctx.match_pairs(pairs, ratio=0.8, cross_check=cc, max_distance=md)
                    assert_route(gpu_ctx.profile(), mode, 0.8, len(pairs), i8_expected=(mode == I8))
                    compare_lists(res, imgs, pairs, int_ref(0.8, cc, md), (mode, md, cc))
    finally:
        gpu_ctx.set_prefilter(True)
        gpu_ctx.clear_images()


def test_byte_extremes_and_the_widest_digit_spread(gpu_ctx):
    """All-0 / all-255 rows and -128 against +127; stores whose h range is the widest the sixteen digits centre (integer cores)
    and one more (not a byte store for the integer path: fp16 cores), same bits as the exact reference."""
    (A, B), pairs = ef.byte_extreme_fixture()
    stores, _ = ef.digit_spread_fixture()
    cases = [("extreme", [A, B], pairs, True)] + [(k, v, np.array([[0, 1], [1, 0]], np.int32), k == "widest") for k, v in stores.items()]
    try:
        for name, imgs, prs, on_i8 in cases:
            for as_float in (False, True):
                upload(gpu_ctx, imgs, as_float)
                for mode in (I8, F16, BRUTE):
                    gpu_ctx.set_prefilter(mode)
                    for cc in (True, False):
                        res = gpu_ctx.match_pairs(prs, ratio=0.8, cross_check=cc, max_distance=1e9)
                        prof = gpu_ctx.profile()
                        if name == "extreme" and mode != BRUTE and not (mode == I8 and on_i8) and prof["fallback_pairs"]:
                            # eps ~ 1.5e-3 (|a|^2 + |b|^2) ~ 2.5e4 at these norms on the fp16 cores: a candidate-list overflow
                            # may send a pair to brute force, which is the documented way out; the bits must not change
                            assert prof["prefilter_pairs"] + prof["fallback_pairs"] == len(prs), prof
                        else:
                            assert_route(prof, mode, 0.8, len(prs), i8_expected=(mode == I8 and on_i8))
                        compare_lists(res, imgs, prs, int_ref(0.8, cc, 1e9), (name, as_float, mode, cc))
                compare_knn(gpu_ctx, imgs, prs[:1], io.knn2, name)
    finally:
        gpu_ctx.set_prefilter(True)
        gpu_ctx.clear_images()


# ------------------------------------------------------------------------------------------------ 2. floats: every route
FLOAT_ROUTES = ("fine", "coarse", "fp16", "brute")


def float_ctx(monkeypatch, route, order):
    monkeypatch.setenv("MSFM_Q8", "2")                      # (route Q on small images too)
    monkeypatch.setenv("MSFM_Q8_DIRECT", "0" if route == "coarse" else "1")
    ctx = _lib.Context(0)
    ctx.set_accum_order(order)
    ctx.set_prefilter({"fine": 1, "coarse": 1, "fp16": 2, "brute": 0}[route])
    return ctx


def assert_float_route(prof, route, ratio):
    assert_route(prof, BRUTE if route == "brute" else F16, ratio, 2)
    twins = route in ("fine", "coarse") and ratio <= 0.95
    assert (prof["sweep1_q8_launches"] >= 1) == twins, (route, ratio, prof)
    assert (prof["sweep1b_launches"] >= 1) == (twins and route == "coarse"), (route, ratio, prof)


def certified_count(oracle, A, B, ratio, cc, md, order):
    """The order certificate of one pair as tests/test_gpu_certificate.py states it, from the oracle's kNN arrays: forward rows
    within the reassociation bound of a flip, + reverse rows when cross-checking.  -> (count, forward row mask)."""
    fi, fd0, _, fd1 = oracle.knn2(A, B, order=order)
    fwd = predicate(fi, fd0, fd1, ratio, md, True)
    n = int(fwd.sum())
    if cc:
        ri, rd0, _, rd1 = oracle.knn2(B, A, order=order)
        n += int(predicate(ri, rd0, rd1, ratio, md, False).sum())
    return n, fwd


@pytest.mark.parametrize("order", [_lib.ORDER_SSE4X4, _lib.ORDER_AVX2_FMA, _lib.ORDER_AVX512_FMA])
def test_float_ratio_ladders_and_distance_cuts_on_every_route(monkeypatch, oracle, order):
    """Per planted row, ratio = the float at which the oracle's decision flips and the float below it (rows near 0.8, the closest
    below and above 0.95, near 0.99), a row whose flip IS the compact / dense switch (dropped at 0.95, kept at the next float), the
    switch ratios themselves; max_distance on a planted d0 and one double either side.  Route Q fine / coarse twins, fp16, brute force,
    under the given accumulation order.  The order certificate of every call equals the count the oracle's kNN arrays give, and that
    count includes each planted row on its flip."""
    imgs, k_sw, _ = ef.plant_switch_row(ef.float_ladder_fixture(top=0.4375))
    A, B = imgs
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    _, d0, _, d1 = oracle.knn2(A, B, order=order)
    r = np.where(np.arange(len(A)) == k_sw, np.nan, d0 / d1)
    below, above = np.where(r < 0.95, r, -1.0), np.where(r > 0.95, r, 9.0)
    rows = [int(np.nanargmin(np.abs(r - 0.8))), int(np.argmax(below)), int(np.argmin(above)), int(np.nanargmin(np.abs(r - 0.99)))]
    flips = [ef.flip_ratio(d0[k], d1[k]) for k in rows]
    assert float(flips[1]) <= 0.95 < float(flips[2])     # those two rows flip on either side of the switch
    ladder = [(float(f), [k]) for f, k in zip(flips, rows)] + [(float(ef.nextf(f, 0)), [k]) for f, k in zip(flips, rows)]
    ladder += [(x, [k_sw] if x in (RATIOS[1], RATIOS[2]) else []) for x in RATIOS]
    dc = float(d0[rows[0]])
    cuts = (0.7, dc, float(np.nextafter(dc, 0)), float(np.nextafter(dc, np.inf)))
    for route in FLOAT_ROUTES:
        with float_ctx(monkeypatch, route, order) as ctx:
            for k, x in enumerate(imgs):
                ctx.upload_image(k, x)
            for ratio, on_flip in ladder:
                for cc in (True, False):
                    for md in (cuts if ratio == RATIOS[0] else cuts[:1]):
                        res = ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=md)
                        assert_float_route(ctx.profile(), route, ratio)
                        compare_lists(res, imgs, pairs, c_ref(oracle, ratio, cc, md, order), (route, ratio, cc, md))
                        cert = ctx.order_certificate(2)
                        for p, (i, j) in enumerate(pairs):
                            n, fwd = certified_count(oracle, imgs[i], imgs[j], ratio, cc, md, order)
                            assert cert[p] == n, (route, ratio, cc, md, p, cert[p], n)
                            if p == 0:
                                assert fwd[on_flip].all(), (route, ratio, on_flip)
            compare_knn(ctx, imgs, pairs[:1], lambda x, y: oracle.knn2(x, y, order=order), route)


# ------------------------------------------------------------------------------------------------ 3. worst-case roundings
@pytest.mark.parametrize("prefilter", [1, 2])
def test_fp16_worst_case_rounding_ladder(gpu_ctx, oracle, prefilter):
    """Coherent fp16 rounding errors at 50 % or more of the row's bound (tests/test_edge_fixtures.py asserts it in a model of the
    sweep), a third neighbour on a ladder of 0.05 .. 20 times the error either side."""
    imgs, pairs, _ = ef.fp16_worst_fixture()
    upload(gpu_ctx, imgs)
    try:
        gpu_ctx.set_prefilter(prefilter)
        for ratio in (0.8, 1.0):
            for cc in (True, False):
                res = gpu_ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=1e9)
                prof = gpu_ctx.profile()
                assert_route(prof, F16, ratio, len(pairs), i8_expected=False)
                assert prof["sweep1_q8_launches"] == 0
                compare_lists(res, imgs, pairs, c_ref(oracle, ratio, cc, 1e9), (ratio, cc))
        compare_knn(gpu_ctx, imgs, pairs, oracle.knn2, "fp16", prefiltered=True)
    finally:
        gpu_ctx.set_prefilter(True)
        gpu_ctx.clear_images()


@pytest.mark.parametrize("level", [0.4375, 0.625])
def test_twin_worst_case_rounding_ladder(monkeypatch, oracle, level):
    """Every element half a twin step from its twin, store maximum exactly at the level (s known), the triangle bound tight, a third
    neighbour on the ladder: route Q with direct thresholds must return the oracle's bits."""
    imgs, pairs, _ = ef.twin_worst_fixture(level)
    with float_ctx(monkeypatch, "fine", 0) as ctx:
        for k, x in enumerate(imgs):
            ctx.upload_image(k, x)
        for ratio in (0.8, 0.95):
            for cc in (True, False):
                res = ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=1e9)
                prof = ctx.profile()
                assert_route(prof, F16, ratio, len(pairs))
                assert prof["sweep1_q8_launches"] >= 1 and prof["sweep1b_launches"] == 0, prof
                compare_lists(res, imgs, pairs, c_ref(oracle, ratio, cc, 1e9), (level, ratio, cc))
        compare_knn(ctx, imgs, pairs, oracle.knn2, level, prefiltered=True)


# ------------------------------------------------------------------------------------------------ 4. route thresholds, both sides
def run_both_sides(ctx, oracle, imgs, ratio=0.8):
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    for k, x in enumerate(imgs):
        ctx.upload_image(k, x)
    out = None
    for cc in (True, False):
        res = ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=1e9)
        prof = ctx.profile()
        compare_lists(res, imgs, pairs, c_ref(oracle, ratio, cc, 1e9), cc)
        assert prof["fallback_pairs"] == 0
        out = prof if out is None else out
    return out


@pytest.mark.parametrize("top,twin,direct", [(1.0, True, False), (float(ef.nextf(1.0, 2)), False, False),
                                             (0.625, True, True), (float(ef.nextf(0.625, 1)), True, False)])
def test_twin_level_thresholds(monkeypatch, oracle, top, twin, direct):
    """Store maximum exactly 1 (twins) and the float above (none); exactly 0.625 (direct thresholds) and the float above (sweep 1')."""
    imgs = ef.float_ladder_fixture(top=top if top <= 1.0 else 1.0)
    if top > 1.0:
        imgs[1][3, 5] = F32(top)
    with float_ctx(monkeypatch, "fine", 0) as ctx:
        prof = run_both_sides(ctx, oracle, imgs)
    assert prof["prefilter_pairs"] == 2
    assert (prof["sweep1_q8_launches"] >= 1) == twin, prof
    assert (prof["sweep1b_launches"] >= 1) == (twin and not direct), prof


def _scaled_pair(seed, scale):
    imgs = ef.float_ladder_fixture(seed=seed, n=120, top=None)
    return [np.ascontiguousarray(x * F32(scale)) for x in imgs]


@pytest.mark.parametrize("case", ["f16safe_at", "f16safe_above", "norms_8x", "norms_8x_ulp", "k15_at", "k15_below",
                                  "kmin_at", "kmin_below"])
def test_prefilter_safety_thresholds(gpu_ctx, oracle, case):
    """Norm maxima exactly 8x apart and 8x + an ulp; 0.5 nrm_max a power of two at the k = 15 limit of c = 2^k and the float below,
    and at k = -24 (clamped below): both sides give the oracle's bits, prefiltered where the rule allows it, brute force where not.
    |value| at 6e4 and the float above (kF16Safe): kF16Safe never decides -- a value >= 2^14 already makes 0.5 nrm_max >= 2^27,
    i.e. k > 15 -- so both of those cases take brute force for the k limit, and they check only that the result is
    the oracle's, not the 6e4 threshold itself."""
    big = {"f16safe_at": F32(6e4), "f16safe_above": ef.nextf(6e4, 1e9)}
    if case in big:
        imgs = _scaled_pair(51, 3e4)
        imgs[0][0, :] = 0
        imgs[0][0, 0] = big[case]
        use = False
    elif case.startswith("norms"):
        imgs = _scaled_pair(52, 1.0)
        imgs[1][0, :] = 0
        imgs[1][0, :2] = 1.0                                   # |row|^2 = 2 exactly: image 1's maximum
        imgs[0][0, :] = 0
        imgs[0][0, 0] = 4.0                                    # 16 = 8 x 2
        if case == "norms_8x_ulp":
            imgs[0][0, 1] = F32(0.0014)                        # 16 + 1.96e-6 rounds to 16 + one ulp
            assert F32(F32(16) + F32(0.0014) ** 2) == ef.nextf(16, 17)
        use = case == "norms_8x"
    else:
        top = {"k15_at": F32(16384), "k15_below": ef.nextf(16384, 0), "kmin_at": F32(2.0 ** -6), "kmin_below": ef.nextf(2.0 ** -6, 0)}[case]
        scale = 4000.0 if case.startswith("k15") else 2.0 ** -8
        imgs = _scaled_pair(53, scale)
        for x in imgs:
            x[0, :] = 0
            x[0, 0] = top                                      # 0.5 |row|^2 = 2^27 (k = 16) / 2^-13 (k = -24) or just below
        use = case != "k15_at"
    try:
        gpu_ctx.set_prefilter(2)
        prof = run_both_sides(gpu_ctx, oracle, imgs)
        assert prof["prefilter_pairs"] == (2 if use else 0), (case, prof)
        if not use:
            assert prof["dist_kernel_launches"] >= 1, (case, prof)
    finally:
        gpu_ctx.set_prefilter(True)
        gpu_ctx.clear_images()


@pytest.mark.parametrize("value,is_bytes", [(255.5, False), (256.0, False), (-0.0, True)])
def test_float_upload_of_byte_values_edges(gpu_ctx, oracle, value, is_bytes):
    imgs, pairs, _ = ef.byte_boundary_fixture(ratios=(0.8,), per_side=1)
    imgs = [x.astype(F32) for x in imgs[:2]]
    imgs[1][-1, 0] = F32(value)
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    upload(gpu_ctx, imgs)
    try:
        for cc in (True, False):
            res = gpu_ctx.match_pairs(pairs, ratio=0.8, cross_check=cc, max_distance=1e9)
            assert_route(gpu_ctx.profile(), I8, 0.8, 2, i8_expected=is_bytes)
            compare_lists(res, imgs, pairs, c_ref(oracle, 0.8, cc, 1e9), (value, cc))
    finally:
        gpu_ctx.clear_images()
