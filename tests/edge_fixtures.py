"""Adversarial fixtures for the matching routes: rows planted ON the decision edges of the reference and at the worst-case
roundings of the prefilter bounds (DESIGN.md sections 2, 3, 5).  Deterministic and seeded; every generator returns the
descriptors together with what it planted, and tests/test_edge_fixtures.py proves on the CPU that each plant is what it
claims (tests/test_gpu_edges.py then runs every route on them).

Every planted case is one image PAIR of a few rows (query image: the query + a far filler; train image: the planted
neighbours + a far filler), so that no case disturbs another and the reverse direction of the cross check has two rows."""
import numpy as np

F32 = np.float32
F64 = np.float64
DIM = 128
# the constants the bounds are stated with (csrc/msfm_prefilter.hip.h, msfm_sweep_i8.hip.h)
K_EPS_REL = 1.5e-3
K_I8_EPS = 2
K_I8_DIGIT_LO, K_I8_DIGIT_HI = -243968, 245759


def nextf(x, toward):
    return np.nextafter(F32(x), F32(toward), dtype=F32)


def keeps(d0, d1, ratio):
    """The reference's Lowe test: d0 < fl32(ratio * d1), strict."""
    return bool(F32(d0) < F32(F32(ratio) * F32(d1)))


def flip_ratio(d0, d1):
    """The smallest float32 ratio at which the Lowe test keeps (d0, d1) (d1 > 0): one ulp below it, it drops."""
    r = F32(F32(d0) / F32(d1))
    while keeps(d0, d1, nextf(r, 0)):
        r = nextf(r, 0)
    while not keeps(d0, d1, r):
        r = nextf(r, 2)
    return r


# ---------------------------------------------------------------------------------------------------------------- bytes
def byte_boundary_pairs(ratio, s_lo, s_hi):
    """Integer pairs (S0, S1), S0 < S1 in [s_lo, s_hi), with sqrtf(S0) ON fl(ratio * sqrtf(S1)) ("eq": dropped), one ulp
    below it ("below": kept) or one ulp above it ("above": dropped).  -> {side: [(S0, S1), ...]}."""
    r = F32(ratio)
    out = {"eq": [], "below": [], "above": []}
    for s1 in range(max(s_lo, 2), s_hi):
        thr = F32(r * np.sqrt(F32(s1)))
        s = int(float(thr) ** 2)
        for s0 in range(max(0, s - 2), min(s + 3, s1)):
            d = np.sqrt(F32(s0))
            side = "eq" if d == thr else "below" if d == nextf(thr, 0) else "above" if d == nextf(thr, 1e9) else None
            if side:
                out[side].append((s0, s1))
    return out


def _two_squares(n, cap):
    for c in range(min(cap, int(np.sqrt(n))), -1, -1):
        d = int(round(np.sqrt(n - c * c)))
        if d * d == n - c * c and d <= cap:
            return c, d
    return None


def _squares(S, n_coords, cap, rng):
    """n_coords integers in [-cap, cap] whose squares sum to S exactly (random magnitudes and signs): random squares until at most
    ~4 cap^2 is left, then four exact ones (Lagrange) by search."""
    assert n_coords >= 4 and 0 <= S <= n_coords * cap * cap
    for _ in range(50):
        v = np.zeros(n_coords, np.int64)
        rem = S
        for i in range(n_coords - 4):
            if rem <= 3 * cap * cap:
                break
            k = int(np.sqrt(rem / (n_coords - i)) * rng.uniform(0.5, 1.5))
            k = min(cap, max(k, int(np.ceil(np.sqrt(max(rem - (n_coords - i - 1) * cap * cap, 0))))))
            v[i] = k
            rem -= k * k
        done = None
        for a in range(min(cap, int(np.sqrt(rem))), -1, -1):
            for bb in range(min(a, int(np.sqrt(rem - a * a))), -1, -1):
                cd = _two_squares(rem - a * a - bb * bb, cap)
                if cd:
                    done = (a, bb) + cd
                    break
            if done:
                break
        if done is None:
            continue
        v[n_coords - 4:] = done
        assert int((v * v).sum()) == S
        rng.shuffle(v)
        return v * rng.choice([-1, 1], n_coords)
    raise ValueError("cannot write %d as a sum of %d squares <= %d^2" % (S, n_coords, cap))


def _neighbour(qs, S, rng, lo=-128, hi=127, n_coords=64, cap=24):
    """A shifted byte row x' = qs + delta with |delta|^2 = S exactly, inside [lo, hi]."""
    for _ in range(200):
        coords = rng.choice(DIM, n_coords, replace=False)
        dv = _squares(S, n_coords, cap, rng)
        t = qs.copy()
        t[coords] += dv
        if t.min() >= lo and t.max() <= hi:
            return t
    raise ValueError("no neighbour at S = %d" % S)


def _byte_case(q_shift, neighbour_S, rng, filler_S):
    """One planted case from shifted rows (x' = x - 128): query image [q, filler], train image [t_k..., filler]."""
    ts = [_neighbour(q_shift, S, rng) for S in neighbour_S]
    # the fillers: the mirror images of the query / of the first neighbour (|x' - (-x')|^2 = 4 |x'|^2), pushed further out along a
    # coordinate of their own if that is not far enough
    qf = -q_shift.copy()
    tf = -ts[0].copy()
    for f, ref in ((qf, q_shift), (tf, ts[0])):
        c = 0
        while int(((f - ref) ** 2).sum()) < filler_S and c < DIM:
            f[c] = -128 if ref[c] >= 0 else 127
            c += 1
    A = np.stack([q_shift, qf]) + 128
    B = np.stack(ts + [tf]) + 128
    return A.astype(np.uint8), B.astype(np.uint8)


def _small_query(rng, parity, amp=2):
    q = rng.integers(-amp, amp + 1, DIM).astype(np.int64)
    if int((q * q).sum()) % 2 != parity:
        q[0] = 1 if q[0] == 0 else (0 if abs(q[0]) == 1 else q[0] + (1 if q[0] > 0 else -1))
        if int((q * q).sum()) % 2 != parity:
            q[1] ^= 1
    assert int((q * q).sum()) % 2 == parity
    return q


def byte_gap_fixture(seed=11):
    """Group 1: integer S gaps at eps = 2.  For both parities of n'_q = |q'|^2 and both parities of S(t1): neighbours at
    S1, S1 + g, S1 + g + g' with g, g' in {0, 1, 2} (all norm-parity combinations of the candidates follow: n'_t = n'_q + S mod 2).
    Small norms (values 128 +- a few), so that the prune's slack (1e-5 of the norms) is far below the parity bits.  Plus rows
    whose decision at ratio 0.8 lies closer to the boundary than eps: 'window' rows, S0 = the last integer the Lowe test keeps.
    -> (images list, pairs P x 2, planted list of dicts)."""
    rng = np.random.default_rng(seed)
    imgs, pairs, planted = [], [], []
    for pq in (0, 1):
        for s1 in (301, 302):
            for g in (0, 1, 2):
                for g2 in (0, 1, 2):
                    q = _small_query(rng, pq)
                    S = [s1, s1 + g, s1 + g + g2]
                    A, B = _byte_case(q, S, rng, filler_S=4 * max(S) + 64)
                    pairs.append((len(imgs), len(imgs) + 1))
                    imgs += [A, B]
                    planted.append({"kind": "gap", "query_parity": pq, "S": S, "gaps": (g, g2), "row": 0, "neighbours": [0, 1, 2]})
    # window rows: d0 kept by the Lowe test at 0.8 by less than the parity bits (odd query norm: S~ = S - 1 for odd S0, S1 - 2 for
    # even S1)
    r = F32(0.8)
    n_window = 0
    for s1 in range(200, 2000, 2):
        thr = F32(r * np.sqrt(F32(s1)))
        s0 = int(float(thr) ** 2) + 2
        while not (np.sqrt(F32(s0)) < thr):
            s0 -= 1
        if s0 % 2 == 0 or float(r) ** 2 * s1 - s0 > 0.25:     # S~0 = S0 - 1 must lie within the parity bits of the boundary
            continue
        q = _small_query(rng, 1)
        S = [s0, s1, s1 + 40]
        A, B = _byte_case(q, S, rng, filler_S=4 * max(S) + 64)
        pairs.append((len(imgs), len(imgs) + 1))
        imgs += [A, B]
        planted.append({"kind": "window", "query_parity": 1, "S": S, "gaps": None, "row": 0, "neighbours": [0, 1, 2], "ratio": 0.8})
        n_window += 1
        if n_window == 6:
            break
    return imgs, np.asarray(pairs, np.int32), planted


def byte_boundary_fixture(seed=12, ratios=(0.8, 0.95), per_side=3):
    """Group 2 for bytes: per ratio, integer (S0, S1) with sqrtf(S0) ON / one ulp below / one ulp above fl(ratio sqrtf(S1))
    (byte_boundary_pairs), realised as byte rows (third neighbour at S1 + 50).  -> (images, pairs, planted)."""
    rng = np.random.default_rng(seed)
    imgs, pairs, planted = [], [], []
    for ratio in ratios:
        cand = byte_boundary_pairs(ratio, 400, 12000)
        for side in ("eq", "below", "above"):
            picks = cand[side]
            idx = np.linspace(0, len(picks) - 1, min(per_side, len(picks))).astype(int)
            for k in idx:
                s0, s1 = picks[k]
                q = rng.integers(-6, 7, DIM).astype(np.int64)
                S = [s0, s1, s1 + 50]
                A, B = _byte_case(q, S, rng, filler_S=4 * max(S) + 64)
                pairs.append((len(imgs), len(imgs) + 1))
                imgs += [A, B]
                planted.append({"kind": "ratio", "ratio": float(F32(ratio)), "side": side, "S": S, "row": 0, "neighbours": [0, 1, 2]})
    return imgs, np.asarray(pairs, np.int32), planted


def byte_extreme_fixture(seed=13):
    """Extreme byte rows: all 0, all 255 (shifted norms 2^21 and 127^2 * 128), x' = -128 against +127 in one coordinate, and
    near neighbours of each.  -> (images, pairs)."""
    rng = np.random.default_rng(seed)
    # the other rows far from 128 (|x'| >= 107), so that the h range of each store stays within the sixteen digits' reach
    far = np.concatenate([np.arange(0, 21), np.arange(235, 256)])
    A = rng.choice(far, (40, DIM)).astype(np.uint8)
    B = rng.choice(far, (40, DIM)).astype(np.uint8)
    B[4:] = np.clip(A[4:].astype(np.int64) + rng.integers(-2, 3, (36, DIM)), 0, 255)   # near-duplicates
    A[0], A[1] = 0, 255
    B[0], B[1] = 0, 255
    B[2] = 0
    B[2, :3] = 1                        # S = 3 from the all-0 query
    B[3] = 255
    B[3, :2] = 254                      # S = 2 from the all-255 query
    A[2] = 0
    A[2, 5] = 255                       # -128 against +127 in one coordinate of B[0]: S = 255^2
    A[3] = 255
    A[3, 7] = 0
    return [A, B], np.asarray([(0, 1), (1, 0)], np.int32)


def _row_with_norm(target, rng):
    """A shifted byte row with n' = |x'|^2 = target exactly."""
    v = _squares(target, DIM, 127, rng)
    v[v == 128] = 127
    assert int((v * v).sum()) == target and v.min() >= -128 and v.max() <= 127
    return v


def digit_spread_fixture(seed=14):
    """Byte images whose h = floor(n'/2) spread is the widest digit_centre accepts (D_max) and one more (D_max + 1), both with
    h_min = 0 (an all-128 row).  -> (dict name -> images list [A, B]), spreads."""
    rng = np.random.default_rng(seed)
    d_max = widest_digit_spread()
    base = rng.integers(88, 169, (60, DIM)).astype(np.int64) - 128
    out = {}
    for name, D in (("widest", d_max), ("one_more", d_max + 1)):
        A = base.copy()
        A[0] = 0
        A[1] = _row_with_norm(2 * D, rng)
        A[2] = A[1]                                             # a duplicate: a tie for the reverse direction
        B = base.copy() + rng.integers(-1, 2, base.shape)       # near-duplicates: short candidate lists on the fp16 cores too
        B = np.clip(B, -128, 127)
        B[0] = A[1]
        B[1] = 0
        B[1, :4] = 1
        out[name] = [(A + 128).astype(np.uint8), (B + 128).astype(np.uint8)]
    return out, (d_max, d_max + 1)


def digit_centre(hmin, hmax):
    """msfm_store_host.hip.h digit_centre on integer h: the centre, or None when sixteen digits cannot represent H0 - h."""
    c = (hmin + hmax) // 2
    if hmin <= hmax and c - hmax >= K_I8_DIGIT_LO and c - hmin <= K_I8_DIGIT_HI:
        return c
    return None


def widest_digit_spread():
    lo, hi = 0, 1 << 21
    while lo < hi:      # the largest D with a centre for h in [0, D]
        mid = (lo + hi + 1) // 2
        if digit_centre(0, mid) is not None:
            lo = mid
        else:
            hi = mid - 1
    return lo


def digits_represent(V):
    """st_digits (msfm_store.hip.h) restated: the sixteen signed digits of V, and whether sum c_k d_k == V."""
    Wp = (V + 128) >> 7
    d = [V - (Wp << 7)]
    R = -Wp
    for _ in range(15):
        x = max(-128, min(127, R))
        d.append(x)
        R -= x
    return d, d[0] - 128 * sum(d[1:]) == V and -128 <= d[0] <= 127


# ---------------------------------------------------------------------------------------------------------------- floats
def float_ladder_fixture(seed=21, n=160, top=1.0):
    """Group 2 for floats: RootSIFT-like query rows (values in [0, 1] -> byte twins), each with two train neighbours at noise scales
    whose ratio is spread over (0.55, 1.05), so that rows flip anywhere between the ratios the routes switch at.  The ratios at which
    planted rows flip are taken from the oracle in the tests (flip_ratio).  The store maximum is exactly `top`."""
    from monocularsfm_amd import synth
    rng = np.random.default_rng(seed)
    A = synth.rootsift_images(1, [n], seed=seed, n_proto=4 * n, sigma=0.05)[0].astype(F64)
    rho = rng.uniform(0.55, 1.05, n)
    s0 = rng.uniform(0.04, 0.12, n)
    B = np.concatenate([np.abs(A + rng.normal(0, 1, A.shape) * (s0 / np.sqrt(DIM))[:, None]),
                        np.abs(A + rng.normal(0, 1, A.shape) * (s0 / rho / np.sqrt(DIM))[:, None])])
    imgs = [A, B[rng.permutation(2 * n)]]
    if top is None:
        return [x.astype(F32) for x in imgs]
    m = max(float(x.max()) for x in imgs)
    imgs = [np.minimum(x * (top / m), top).astype(F32) for x in imgs]
    k = np.unravel_index(int(np.argmax(imgs[0])), imgs[0].shape)
    imgs[0][k] = F32(top)
    return imgs


def plant_switch_row(imgs, ratio=0.95):
    """Append to a float pair (query image, train image) a query whose Lowe decision flips exactly at the compact / dense switch:
    dropped at fl(ratio), kept at the next float up.  Its two neighbours differ from it in ONE coordinate each (the query is 0
    there), so d = sqrtf(fl(delta^2)) under every accumulation order.  -> (imgs, query row, (first, second) train rows)."""
    A, B = (np.asarray(x, F32) for x in imgs)
    r, r_up = F32(ratio), nextf(ratio, 2)
    # the query: the first query row with its coordinates rotated by half (an unrelated pattern: ~1 from every row, and a twin norm
    # like theirs -- a row of zeros would widen the twins' h range beyond the digits' reach and cost the image its twin), 0 where
    # its neighbours differ from it
    q = np.roll(A[0], DIM // 2).copy()
    q[10] = q[11] = 0
    d1_delta = F32(0.3)
    while True:
        d1 = np.sqrt(F32(d1_delta * d1_delta))
        thr, thr_up = F32(r * d1), F32(r_up * d1)
        if thr < thr_up:
            break
        d1_delta = nextf(d1_delta, 1)
    d0_delta = thr
    while np.sqrt(F32(d0_delta * d0_delta)) != thr:
        d0_delta = nextf(d0_delta, 1 if np.sqrt(F32(d0_delta * d0_delta)) < thr else 0)
    t0, t1 = q.copy(), q.copy()
    t0[10], t1[11] = d0_delta, d1_delta
    return [np.vstack([A, q[None]]), np.vstack([B, t0[None], t1[None]])], len(A), (len(B), len(B) + 1)


def fp16_model_s(a, b):
    """S~ as the fp16 sweep forms it, in float64: exact fp32 norms (float64 here), operands rounded to fp16, exact products,
    float64 sums.  -> (S~, S exact in float64)."""
    a64, b64 = np.asarray(a, F64), np.asarray(b, F64)
    ah, bh = np.asarray(a, np.float16).astype(F64), np.asarray(b, np.float16).astype(F64)
    na, nb = (a64 * a64).sum(-1), (b64 * b64).sum(-1)
    return na + nb - 2.0 * (ah * bh).sum(-1), ((a64 - b64) ** 2).sum(-1)


LADDER = (-20.0, -5.0, -2.0, -1.0, -0.5, -0.2, -0.05, 0.05, 0.2, 0.5, 1.0, 2.0, 5.0, 20.0)


def snap_fp16(v, up):
    """fp32 values next to v that sit just short of (up=False: round DOWN to fp16) or just past (up=True: round UP) an fp16 rounding
    midpoint: the rounding error is almost half an fp16 ulp, in the chosen direction."""
    v = np.asarray(v, F64)
    lo = v.astype(np.float16)
    lo = np.where(lo.astype(F64) > v, np.nextafter(lo, np.float16(-np.inf)), lo)
    hi = np.nextafter(lo, np.float16(np.inf))
    mid = (lo.astype(F64) + hi.astype(F64)) / 2
    x = mid.astype(F32)
    for _ in range(8):
        x = np.where(x.astype(np.float16) == (hi if up else lo), x, np.nextafter(x, F32(np.inf) if up else F32(-np.inf)))
    assert (x.astype(np.float16) == (hi if up else lo)).all()
    return x


def fp16_worst_fixture(seed=31, ladder=LADDER):
    """Group 3, fp16: values just above 1 (no twins: the fp16 sweep is the one under test; the relative half-ulp of fp16 is
    largest there), a few coordinates further out to give the neighbours distance.  The query and its neighbour t_dn sit just short
    of an fp16 rounding midpoint (they round DOWN by almost half an ulp: a~.b~ errs low coherently, S~ exceeds S by E >= half of
    kEpsRel (na + max nb), the row's bound in the kernel); the neighbours t_up / t_lad sit just past one (they round UP: S~ - S ~ 0).  S(t_up) = S(t_dn) - E / 2,
    S(t_lad) = S(t_dn) + lam E for lam on the ladder: where lam < 1, S~ ranks t_lad before t_dn although t_dn is the true second
    neighbour, and only the full eps keeps t_dn a candidate (query image: q, decoys of t_dn, fillers; train image: t_dn, t_up,
    t_lad, filler).  -> (images, pairs, planted)."""
    rng = np.random.default_rng(seed)
    u = 2.0 ** -10
    imgs, pairs, planted = [], [], []
    for lam in ladder:
        qv = 1.0 + rng.integers(8, 40, DIM) * u
        q = snap_fp16(qv, False)
        dv = rng.integers(-6, 7, DIM) * u
        dv[:12] = 0.9                                         # S(t_dn) ~ 10 > 20 E: room below for the ladder's negative rungs
        t_dn = snap_fp16(q.astype(F64) + dv, False)
        s_dn = float(((t_dn.astype(F64) - q) ** 2).sum())
        E = float(fp16_model_s(q, t_dn)[0] - s_dn)

        def up_row(target):
            # rounding UP; coordinate 4 is tuned to the target S, then the snap's residue is corrected on coordinate 5
            d = rng.integers(-6, 7, DIM) * u
            d[:12] = 0.9
            t = snap_fp16(q.astype(F64) + d, True)
            for c in list(range(12)) + [0, 1]:
                rest = float(((t.astype(F64) - q) ** 2).sum()) - float((t[c].astype(F64) - q[c]) ** 2)
                need = max(target - rest, 0.0)
                t[c] = snap_fp16(np.array([float(q[c]) + np.sqrt(need)]), True)[0]
            return t
        t_up = up_row(s_dn - 0.5 * E)
        t_lad = up_row(s_dn + lam * E)
        # the train filler: 24 coordinates of its own moved DOWN by 0.9 (S ~ 19 from t_dn, ~ 29 from q), so its norm is below the
        # planted rows' (the kernel's bound for a row uses the largest norm of the other image: a filler further out would inflate it
        # and leave the planted error a smaller share of the bound)
        shift = np.zeros(DIM)
        shift[12:36] = -0.9
        filler_t = snap_fp16(t_dn.astype(F64) + shift, False)
        # the query image: q at row 0, DECOYS beyond t_dn as seen from q (S ~ 0.25 .. 0.36 S(t_dn) from t_dn, > 2 S(t_dn) from q) at
        # rows 1-5 and 64-71, fillers elsewhere.  Sweep 1 keeps a column's minima per class of query rows (csrc/msfm_sweep.hip.h:
        # the wave's parity x the MFMA row interleave): with decoys in every class, t_dn's column threshold does not reach back to q
        A = np.empty((72, DIM), F32)
        decoys = list(range(1, 6)) + list(range(64, 72))
        away = t_dn.astype(F64) - q
        for r in range(1, 72):
            if r in decoys:
                A[r] = snap_fp16(t_dn.astype(F64) + rng.uniform(0.5, 0.6) * away + rng.integers(-3, 4, DIM) * u, False)
            else:
                sh = np.zeros(DIM)
                sh[rng.choice(np.arange(24, DIM), 12, replace=False)] = 1.3
                A[r] = snap_fp16(q.astype(F64) + sh, False)
        A[0] = q
        B = np.stack([t_dn, t_up, t_lad, filler_t]).astype(F32)
        pairs.append((len(imgs), len(imgs) + 1))
        imgs += [A, B]
        planted.append({"kind": "fp16", "lam": lam, "E": E, "row": 0, "t_dn": 0, "t_up": 1, "t_lad": 2, "decoys": decoys})
    return imgs, np.asarray(pairs, np.int32), planted


def twin_scale(level):
    """(s, inv) of route Q at a twin level (msfm_store_host.hip.h build_twins): fp32 255 / m and m / 255."""
    return F32(F32(255.0) / F32(level)), F32(F32(level) / F32(255.0))


def twin_model(x, level):
    """Byte twins of float rows: q = rint(s x) (ties to even), the per-row error norm |x - q inv| (float64)."""
    s, inv = twin_scale(level)
    x = np.asarray(x, F32)
    q = np.rint((x * s).astype(F32)).astype(np.int64)
    err = np.sqrt(((x.astype(F64) - q * F64(inv)) ** 2).sum(-1))
    return q, err


def twin_worst_fixture(level, seed=41, ladder=LADDER[4:]):
    """Group 3, twins: every element at (k + 1/2) / s -+ a few fp32 ulps (the twin rounds down for the query and its neighbour
    t_dn, up for t_up / t_lad), so every row's twin error norm is ~ 0.5 inv sqrt(128), the most there is.  The query and t_dn differ
    by the same integer number of twin steps in every coordinate, so |a^ - b^| = |a - b| -+ (e_a + e_b): the triangle bound is tight.
    Each pair holds one row at exactly `level` (the store maximum fixes s).  S(t_lad) = S(t_dn) + lam G, G = the modelled gap
    |S^ inv^2 - S|.  -> (images, pairs, planted)."""
    rng = np.random.default_rng(seed)
    s, inv = twin_scale(level)
    kmax = int(np.floor(float(level) * float(s))) - 1
    imgs, pairs, planted = [], [], []

    def at(k, up):
        # the fp32 value nearest (k + 1/2) / s whose twin rounds to k (up=False) or k + 1 (up=True)
        x = ((k + 0.5) / F64(s)).astype(F32)
        want = k + 1 if up else k
        for _ in range(16):
            ok = np.rint((x * s).astype(F32)) == want
            if ok.all():
                break
            x = np.where(ok, x, np.nextafter(x, F32(2) if up else F32(0)))
        assert (np.rint((x * s).astype(F32)) == want).all()
        return x

    for lam in ladder:
        k_q = rng.integers(kmax // 4, kmax // 2, DIM)
        q = at(k_q, False)
        step = int(rng.integers(2, 4))
        t_dn = at(k_q + step, True)                      # every coordinate moves the same way: the errors add up along (t - q)
        s_dn = float(((t_dn.astype(F64) - q) ** 2).sum())
        qq, _ = twin_model(q, level)
        qt, _ = twin_model(t_dn, level)
        G = abs(float(((qq - qt) ** 2).sum()) * float(inv) ** 2 - s_dn)
        # t_lad: k_q + m on n coordinates (the twin step is 1 / s), elements rounding up: S ~ n m^2 / s^2
        target = s_dn + lam * G
        units = target * float(s) ** 2
        m = max(1, int(np.ceil(np.sqrt(units / DIM))))
        k_l = k_q.copy()
        k_l[rng.choice(DIM, min(DIM, int(round(units / (m * m)))), replace=False)] += m
        t_lad = at(k_l, True)
        # the fillers: the query / t_dn with 16 coordinates at exactly the level (the store maximum); like the planted rows they keep
        # the twins' h range within the digits' reach (a row of zeros would not)
        filler_q = q.copy()
        filler_q[:16] = F32(level)
        filler_t = t_dn.copy()
        filler_t[16:32] = F32(level)
        A = np.stack([q, filler_q]).astype(F32)
        B = np.stack([t_dn, t_lad, filler_t]).astype(F32)
        pairs.append((len(imgs), len(imgs) + 1))
        imgs += [A, B]
        planted.append({"kind": "twin", "lam": lam, "G": G, "row": 0, "t_dn": 0, "t_lad": 1})
    return imgs, np.asarray(pairs, np.int32), planted
