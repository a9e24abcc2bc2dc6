"""The adversarial fixtures of tests/edge_fixtures.py realise what they claim (CPU: the exact-integer reference, the C oracle and a
float64 model of the fp16 sweep).  tests/test_gpu_edges.py runs every matching route on them."""
import numpy as np
import pytest

import edge_fixtures as ef
from oracle import int_oracle as io

F32 = np.float32


def test_byte_gap_fixture_plants_integer_gaps_under_every_parity():
    imgs, pairs, planted = ef.byte_gap_fixture()
    combos = set()
    for (i, j), p in zip(pairs, planted):
        A, B = imgs[i], imgs[j]
        S = io.s_matrix(A, B)
        assert list(S[0, :3]) == p["S"]
        assert S[0, 3] > max(p["S"]) and S[1, :3].min() > max(p["S"])      # the fillers are farther than every planted neighbour
        assert (io.s_matrix(B, A)[:3, 1] > S[0, :3]).all()                 # the reverse direction finds the query first
        nq = int(((A[0].astype(np.int64) - 128) ** 2).sum())
        nt = ((B[:3].astype(np.int64) - 128) ** 2).sum(1)
        assert nq % 2 == p["query_parity"]
        if p["kind"] == "gap":
            assert (p["S"][1] - p["S"][0], p["S"][2] - p["S"][1]) == p["gaps"]
            combos.add((nq % 2, int(nt[0]) % 2, p["gaps"]))
        # S~ = S - (n'_q mod 2) - (n'_t mod 2): within eps = 2 below S, never above
        s_tilde = S[0, :3] - nq % 2 - nt % 2
        assert ((S[0, :3] - s_tilde >= 0) & (S[0, :3] - s_tilde <= ef.K_I8_EPS)).all()
    assert len(combos) == 2 * 2 * 9          # both query parities x both neighbour parities x every gap combination


def _pf_dead_model(s0, s1, nrm, other_max, eps, ratio, max_distance=1e9):
    """pf_dead (csrc/msfm_prefilter.hip.h) in fp32."""
    s0, s1, nrm, other_max, eps = (F32(v) for v in (s0, s1, nrm, other_max, eps))
    tiny = F32(1e-5) * (abs(s0) + abs(s1) + nrm + other_max)
    s0lb = max(F32(s0 - eps - tiny), F32(0))
    s1ub = F32(s1 + eps + tiny)
    d0lb = F32(np.sqrt(s0lb) * F32(1 - 1e-6))
    ratio_fails = d0lb >= F32(F32(ratio) * np.sqrt(s1ub) * F32(1 + 1e-5))
    return bool(ratio_fails or d0lb > F32(max_distance) * F32(1 + 1e-5))


def test_byte_window_rows_need_the_parity_bits():
    """The 'window' rows match at ratio 0.8, and the prune's proof declares them dead if eps were 0 instead of 2: only the parity
    bits of h = floor(n'/2) keep them alive."""
    imgs, pairs, planted = ef.byte_gap_fixture()
    n_window = 0
    for (i, j), p in zip(pairs, planted):
        if p["kind"] != "window":
            continue
        A, B = imgs[i], imgs[j]
        q, t, _ = io.compute_matches(A, B, 0.8)
        assert 0 in q.tolist(), "the window row matches"
        S = io.s_matrix(A, B)[0]
        nq = int(((A[0].astype(np.int64) - 128) ** 2).sum())
        nt = ((B.astype(np.int64) - 128) ** 2).sum(1)
        st = np.sort(S - nq % 2 - nt % 2)
        norms = 2 * (nt // 2)
        args = (st[0], st[1], 2 * (nq // 2), norms.max())
        assert not _pf_dead_model(*args, eps=2, ratio=0.8)
        assert _pf_dead_model(*args, eps=0, ratio=0.8)
        n_window += 1
    assert n_window >= 3


def test_byte_boundary_pairs_sit_on_the_lowe_boundary():
    imgs, pairs, planted = ef.byte_boundary_fixture()
    sides = set()
    for (i, j), p in zip(pairs, planted):
        A, B = imgs[i], imgs[j]
        i0, d0, i1, d1 = io.knn2(A, B)
        assert (i0[0], i1[0]) == (0, 1)
        assert list(io.s_matrix(A, B)[0, :3]) == p["S"]
        thr = F32(F32(p["ratio"]) * d1[0])
        want = {"eq": thr, "below": ef.nextf(thr, 0), "above": ef.nextf(thr, 1e9)}[p["side"]]
        assert d0[0] == want
        q, _, _ = io.compute_matches(A, B, p["ratio"])
        assert (0 in q.tolist()) == (p["side"] == "below")                 # adjacent rungs flip the reference's decision
        sides.add((p["ratio"], p["side"]))
    assert len(sides) == 6


def test_byte_extreme_rows():
    (A, B), _ = ef.byte_extreme_fixture()
    S = io.s_matrix(A, B)
    assert S[0, 2] == 3 and S[1, 3] == 2 and S[2, 0] == 255 ** 2
    assert (A[0] == 0).all() and (A[1] == 255).all()
    for x in (A, B):          # still a byte store for the integer cores
        h = ((x.astype(np.int64) - 128) ** 2).sum(1) // 2
        assert ef.digit_centre(int(h.min()), int(h.max())) is not None


def test_digit_range_and_the_widest_spread():
    """st_digits represents exactly [kI8DigitLo, kI8DigitHi]; the fixture's stores span the widest h range digit_centre accepts, and
    one more."""
    for V in (ef.K_I8_DIGIT_LO, ef.K_I8_DIGIT_HI, 0, -1, 12345):
        assert ef.digits_represent(V)[1], V
    assert not ef.digits_represent(ef.K_I8_DIGIT_HI + 1)[1] and not ef.digits_represent(ef.K_I8_DIGIT_LO - 1)[1]
    stores, (widest, one_more) = ef.digit_spread_fixture()
    assert one_more == widest + 1
    for name, D in (("widest", widest), ("one_more", one_more)):
        A = stores[name][0]
        h = ((A.astype(np.int64) - 128) ** 2).sum(1) // 2
        assert h.min() == 0 and h.max() == D
        c = ef.digit_centre(int(h.min()), int(h.max()))
        assert (c is not None) == (name == "widest")
        if c is not None:
            assert all(ef.digits_represent(c - int(x))[1] for x in (h.min(), h.max()))


def test_fp16_fixture_realises_the_bound():
    """Modelled fp16 sweep: E(t_dn) >= 50 % of kEpsRel (na + max nb) and never above the bound; t_up / t_lad err by < 5 % of E; the
    ladder's S gaps are the claimed multiples of E, so the fp16 order of t_dn and t_lad is the wrong one where lam < 1."""
    imgs, pairs, planted = ef.fp16_worst_fixture()
    for (i, j), p in zip(pairs, planted):
        A, B = imgs[i], imgs[j]
        assert min(A.max(), B.max()) > 1.0 and max(A.max(), B.max()) < 6e4   # no twins, fp16-safe: the fp16 sweep is the one under test
        st, s = ef.fp16_model_s(A[0], B[:3])
        # the kernel's bound for a row: kEpsRel (|a|^2 + the largest |b|^2 of the other image)
        na, nb_max = float((A[0].astype(np.float64) ** 2).sum()), float((B.astype(np.float64) ** 2).sum(1).max())
        E = st[0] - s[0]
        bound = ef.K_EPS_REL * (na + nb_max)
        assert 0.5 * bound <= E <= bound, (p["lam"], E, bound)
        S_all = ((A[0].astype(np.float64) - B) ** 2).sum(1)
        others = np.setdiff1d(np.arange(1, len(A)), p["decoys"])
        assert S_all[3] > S_all[:3].max() + 5
        assert ((A[others].astype(np.float64)[:, None] - B[None, :3]) ** 2).sum(-1).min() > S_all[:3].max() + 5
        # the decoys: t_dn's nearest query-image rows (its column threshold does not reach back to q), far from q
        col = ((A.astype(np.float64) - B[0]) ** 2).sum(1)
        col_bound = ef.K_EPS_REL * (float((B[0].astype(np.float64) ** 2).sum()) + float((A.astype(np.float64) ** 2).sum(1).max()))
        assert col[p["decoys"]].max() + 4 * col_bound < col[0] and col[others].min() > col[0]
        assert ((A[p["decoys"]].astype(np.float64) - A[0]) ** 2).sum(1).min() > S_all[:3].max() + 5
        assert abs(st[1] - s[1]) < 0.05 * E and abs(st[2] - s[2]) < 0.05 * E
        assert abs((s[2] - s[0]) / E - p["lam"]) <= 0.01 + 0.01 * abs(p["lam"])
        assert abs((s[1] - s[0]) / E + 0.5) <= 0.01
        if 0 < p["lam"] < 1:
            assert st[2] < st[0] and s[2] > s[0]


@pytest.mark.parametrize("level", [0.4375, 0.625])
def test_twin_fixture_has_the_largest_error_norms(level):
    imgs, pairs, planted = ef.twin_worst_fixture(level)
    _, inv = ef.twin_scale(level)
    for (i, j), p in zip(pairs, planted):
        A, B = imgs[i], imgs[j]
        assert max(A.max(), B.max()) == F32(level) and min(A.min(), B.min()) >= 0
        for x in (A, B):      # the twins are byte stores the digits can centre (else the image gets no twin)
            h = ((ef.twin_model(x, level)[0] - 128) ** 2).sum(1) // 2
            assert ef.digit_centre(int(h.min()), int(h.max())) is not None
        q_a, e_a = ef.twin_model(A[:1], level)
        q_b, e_b = ef.twin_model(B[:2], level)
        assert (e_a >= 0.8 * 0.5 * float(inv) * np.sqrt(128)).all() and (e_b >= 0.8 * 0.5 * float(inv) * np.sqrt(128)).all()
        # the triangle bound is tight for t_dn: |d^ - d| is within 1 % of e_a + e_b
        d = np.sqrt(((A[0].astype(np.float64) - B[0]) ** 2).sum())
        dh = np.sqrt(((q_a[0] - q_b[0]) ** 2).sum()) * float(inv)
        assert abs(abs(dh - d) - (e_a[0] + e_b[0])) <= 0.01 * (e_a[0] + e_b[0])
        s = ((A[0].astype(np.float64) - B[:2]) ** 2).sum(1)
        assert abs((s[1] - s[0]) - p["lam"] * p["G"]) <= 0.1 * p["G"] + 0.02 * abs(p["lam"]) * p["G"]


def test_float_ladder_fixture_has_rows_near_every_ratio(oracle):
    imgs = ef.float_ladder_fixture()
    assert max(x.max() for x in imgs) == F32(1.0)
    _, d0, _, d1 = oracle.knn2(imgs[0], imgs[1])
    r = d0 / d1
    for lo, hi in ((0.75, 0.8), (0.9, 0.95), (0.95, 1.0)):
        assert ((r > lo) & (r < hi)).sum() >= 2, (lo, hi)
    # flip_ratio: the decision flips between the returned ratio and the float below it
    for k in np.nonzero((r > 0.5) & (r < 1.0))[0][:20]:
        f = ef.flip_ratio(d0[k], d1[k])
        assert ef.keeps(d0[k], d1[k], f) and not ef.keeps(d0[k], d1[k], ef.nextf(f, 0))


@pytest.mark.parametrize("order", [0, 1, 3])
def test_switch_row_flips_between_095_and_the_next_float(oracle, order):
    imgs, k, (t0, t1) = ef.plant_switch_row(ef.float_ladder_fixture(top=0.4375))
    i0, d0, i1, d1 = oracle.knn2(imgs[0], imgs[1], order=order)
    assert (i0[k], i1[k]) == (t0, t1) and d1[k] * 1.5 < np.sort(((imgs[1].astype(np.float64) - imgs[0][k]) ** 2).sum(1))[2] ** 0.5
    assert ef.flip_ratio(d0[k], d1[k]) == ef.nextf(0.95, 1)
    ri0 = oracle.knn2(imgs[1], imgs[0], order=order)[0]
    assert ri0[t0] == k and ri0[t1] == k                 # the cross check keeps it where the ratio test does
    assert max(x.max() for x in imgs) == F32(0.4375)
    for x in imgs:            # both images keep their byte twins: the digits centre their h range
        h = ((ef.twin_model(x, 0.4375)[0] - 128) ** 2).sum(1) // 2
        assert ef.digit_centre(int(h.min()), int(h.max())) is not None
