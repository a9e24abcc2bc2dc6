"""The ratio cap of the reverse thresholds (csrc/msfm_hostutil.h: msfm_ratio_cap_*): with match lists at a ratio up to 0.9 a
column's candidates reach d0 / ratio, not its second neighbour (ratios in (0.9, 0.95] take the compacted sweep 2 with the uncapped
thresholds, the float above 0.95 the dense one: all of them run here); a column that ends without a second candidate passes the Lowe test
by proof (d1 = +inf).  Every route must still return the bits of the C oracle and of the brute-force route, and the same order
certificate -- the reference's test is m[0].distance < ratio * m[1].distance on cv::BFMatcher's two nearest
(/root/reference/src/Feature/FeatureUtils.cpp:141-174).

Two images per job: image 0 with n1 rows (3 blocks of 512 with a partial last one; 17 blocks: the loops behind the 16 register
blocks; 33 blocks: two blocks per mask bit), image 1 with 600.  Rows of image 1 get planted neighbours in image 0, built in the style
of tests/edge_fixtures.py (plant_switch_row: a neighbour differs from its row in ONE coordinate, where the row is 0, so its distance is
sqrtf(fl(delta^2)) = delta under every accumulation order; bytes: edge_fixtures._neighbour at an exact integer S):

  single        the best neighbour and nothing else                           -> no second candidate: the proven pass
  eq / below    a competitor with d0 == fl(ratio * d1) (dropped: it sits just inside the cap and must be found) and with d0 one ulp
                below that (kept: just outside), for each of the ratios, in the best's block and in another one
  tie           two rows at exactly the same distance in two different blocks
  inside / out  a competitor well inside d0 / ratio and one at 1.3 of it, in another block
The rest of both images are unrelated rows (their best and second are alike: dead)."""
import numpy as np
import pytest

import edge_fixtures as ef
from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
N2 = 600
BLOCK = 512                       # kPfWgRows: rows of image 1 per mask block and per compacted work item
PLANT_RATIOS = (0.6, 0.8, 0.95)
DENSE = float(ef.nextf(0.95, 1))  # the compact / dense switch: the float above 0.95 takes the dense sweep 2 (uncapped thresholds)
RATIOS = PLANT_RATIOS + (0.9, DENSE)   # 0.9: the largest capped ratio (msfm_ratio_cap_on); 0.95: compacted, uncapped
KINDS = ("single", "eq_same", "below_same", "eq_other", "below_other", "tie", "inside_other", "outside_other")


def b(a):
    return np.asarray(a).view(np.int32)


def same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(b(x[2]), b(y[2]))


_BYTE_BOUNDS = {}


def byte_bounds():
    """Integer (S0, S1) ON the Lowe boundary of each planted ratio ('eq': dropped) and one ulp below it ('below': kept), once."""
    if not _BYTE_BOUNDS:
        for r in PLANT_RATIOS:
            _BYTE_BOUNDS[r] = ef.byte_boundary_pairs(r, 400, 12000)
            assert _BYTE_BOUNDS[r]["eq"] and _BYTE_BOUNDS[r]["below"]
    return _BYTE_BOUNDS


class Slots:
    """Free rows of image 0 per 512-row block, in a seeded random order."""

    def __init__(self, n1, rng, only_block=None):
        self.nb = (n1 + BLOCK - 1) // BLOCK
        self.free = [list(rng.permutation(np.arange(p * BLOCK, min(n1, (p + 1) * BLOCK)))) for p in range(self.nb)]
        self.only = only_block

    def take(self, block):
        block = self.only if self.only is not None else block
        for k in range(self.nb):     # (a full block -- the partial last one fills up first -- hands on to the next)
            p = (block + k) % self.nb
            if self.free[p]:
                return int(self.free[p].pop()), p
        raise ValueError("image 0 is full")


def plant_job(n1, kind, n_planted=300, one_block=None, seed=5):
    """-> (images [image 0, image 1], per planted column its kind, ratio and the blocks of its rows in image 0)."""
    rng = np.random.default_rng(seed + n1)
    if kind == "float":
        A = synth.rootsift_images(1, [n1], seed=seed + n1, overlap=0.0)[0].copy()
        B = synth.rootsift_images(1, [N2], seed=seed + n1 + 1, overlap=0.0)[0].copy()
    else:
        A = rng.integers(64, 193, (n1, ef.DIM)).astype(np.int64) - 128
        B = rng.integers(64, 193, (N2, ef.DIM)).astype(np.int64) - 128
        bounds = byte_bounds()
    slots = Slots(n1, rng, one_block)
    nb = slots.nb
    cols = rng.choice(N2, n_planted, replace=False)
    planted = []
    for k, t in enumerate(cols):
        what, ratio = KINDS[k % len(KINDS)], PLANT_RATIOS[(k // len(KINDS)) % len(PLANT_RATIOS)]
        blk = (7 * k) % nb
        other = blk if what.endswith("same") else (blk + 1 + k % max(1, nb - 1)) % nb
        rows = []
        if kind == "float":
            B[t, 10:13] = 0
            d1 = F32(rng.uniform(0.2, 0.3))
            thr = F32(F32(ratio) * d1)
            d0 = {"single": F32(rng.uniform(0.1, 0.2)), "tie": F32(rng.uniform(0.1, 0.2)), "eq": thr, "below": ef.nextf(thr, 0),
                  "inside": F32((ratio + 0.3 * (1.0 - ratio)) * d1), "outside": F32(ratio * d1 / 1.3)}[what.split("_")[0]]
            assert np.sqrt(F32(d0 * d0)) == d0 and np.sqrt(F32(d1 * d1)) == d1           # the distances ARE the deltas
            for coord, delta, where in ((10, d0, blk),) + (() if what == "single" else ((11, d0 if what == "tie" else d1, other),)):
                r, p = slots.take(where)
                A[r] = B[t]
                A[r, coord] = delta
                rows.append((r, p))
        else:
            picks = bounds[ratio]["eq" if what.startswith(("eq", "tie", "inside")) else "below"]
            while True:      # (edge_fixtures._squares does not find rows for every S: draw again)
                s0, s1 = picks[int(rng.integers(len(picks)))]
                if what.startswith("inside"):
                    s1 = s0 + max(1, int(0.5 * (s0 / ratio ** 2 - s0)))
                if what.startswith("outside"):
                    s1 = int(s0 / ratio ** 2 * 1.7)
                try:
                    new = [ef._neighbour(B[t], S, rng) for S in (s0,) + (() if what == "single" else (s0 if what == "tie" else s1,))]
                except ValueError:
                    continue
                if len(new) == 1 or not np.array_equal(new[0], new[1]):
                    break
            for x, where in zip(new, (blk, other)):
                r, p = slots.take(where)
                A[r] = x
                rows.append((r, p))
        planted.append({"col": int(t), "kind": what, "ratio": ratio, "rows": rows})
    if kind == "float":
        return [A.astype(F32), B.astype(F32)], planted
    return [(A + 128).astype(np.uint8), (B + 128).astype(np.uint8)], planted


def oracle_lists(oracle, imgs, pairs, ratio, cc, md):
    offs, q, t, d = oracle.match_pairs([np.asarray(x, F32) for x in imgs], pairs, ratio=ratio, cross_check=cc, max_distance=md, nthreads=8)
    return np.asarray(offs), np.stack([q, t], 1), np.asarray(d, F32)


def contexts(monkeypatch, kind):
    """-> [(route name, context, prefilter mode)], the contexts to close.  Route Q's switches are read when a context is created."""
    monkeypatch.setenv("MSFM_Q8", "2")              # route Q on small images too
    monkeypatch.setenv("MSFM_Q8_DIRECT", "1")
    main = _lib.Context(0)
    if kind == "byte":
        return [("brute", main, 0), ("i8", main, 1), ("fp16", main, 2)], [main]
    monkeypatch.setenv("MSFM_Q8_DIRECT", "0")       # the refinement sweep 1' (what a store with values near 1 takes)
    refined = _lib.Context(0)
    return [("brute", main, 0), ("direct", main, 1), ("fp16", main, 2), ("refined", refined, 1)], [main, refined]


def assert_route(prof, route, ratio, n_pairs):
    if route == "brute":
        assert prof["prefilter_pairs"] == 0 and prof["dist_kernel_launches"] >= 1, prof
        return
    compact = ratio <= 0.95
    assert prof["prefilter_pairs"] == n_pairs and prof["fallback_pairs"] == 0, (route, ratio, prof)
    assert (prof["compacted_pairs"] > 0) == compact, (route, ratio, prof)
    assert (prof["sweep1_i8_launches"] >= 1) == (compact and route in ("i8", "direct", "refined")), (route, ratio, prof)
    assert (prof["sweep1_q8_launches"] >= 1) == (compact and route in ("direct", "refined")), (route, ratio, prof)
    assert (prof["sweep1b_launches"] >= 1) == (compact and route == "refined"), (route, ratio, prof)


@pytest.mark.parametrize("kind", ["float", "byte"])
@pytest.mark.parametrize("n1", [1100, 8704, 16896])
def test_capped_reverse_thresholds_return_the_oracles_bits_on_every_route(monkeypatch, oracle, n1, kind):
    imgs, planted = plant_job(n1, kind, n_planted=300 if kind == "float" else 120)    # (exact integer rows are slow to build)
    assert {p["kind"] for p in planted} == set(KINDS)
    assert any(p["kind"] == "tie" and p["rows"][0][1] != p["rows"][1][1] for p in planted)          # a tie across two blocks
    assert any(p["rows"][0][1] == (n1 - 1) // BLOCK for p in planted)                                # a best in the last block
    pairs = np.array([[0, 1], [1, 0]], np.int32)
    md = 0.7 if kind == "float" else 1e9
    routes, owned = contexts(monkeypatch, kind)
    try:
        for ctx in owned:
            for k, x in enumerate(imgs):
                ctx.upload_image(k, x)
        for ratio in RATIOS:
            for cc in (True, False):
                want = oracle_lists(oracle, imgs, pairs, ratio, cc, md)
                assert want[0][-1] >= len(planted) // 8          # the planted rows do match
                brute = None
                for route, ctx, mode in routes:
                    ctx.set_prefilter(mode)
                    got = ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=md)
                    prof = ctx.profile()
                    assert_route(prof, route, ratio, len(pairs))
                    assert same(got, want), (route, ratio, cc)
                    if route == "brute":
                        brute = (got, prof["order_sensitive_rows"])
                    else:
                        assert same(got, brute[0]), (route, ratio, cc)
                        assert prof["order_sensitive_rows"] == brute[1], (route, ratio, cc, prof["order_sensitive_rows"], brute[1])
    finally:
        for ctx in owned:
            ctx.close()


@pytest.mark.parametrize("route", ["direct", "fp16", "refined"])
def test_one_block_per_live_column(monkeypatch, oracle, route):
    """Every planted row of image 0 sits in block 1 (rows 512 .. 1023 of 1100), so every neighbour of a live column within d0 / ratio
    lies in ONE block, and the capped block masks name that block only.

    The bound.  The compacted sweep 2 multiplies, per group, its live rows rounded UP to 512 (a work item is 512 compacted rows) by the
    rows of the streamed range (pf_plan_scan_kernel):
        forward  (one group):            ceil512(live rows of image 0) x 600
        reverse  (one group per block p): ceil512(live columns whose mask has bit p) x rows of block p  (512, 512, 76).
    Live columns: the planted ones, C of them, and nothing else -- an unrelated column has d0 and d1 alike, and the test checks with a
    margin of 0.03 on both distances (more than the twins' 4 x 0.0056 and the fp16 bound's ~0.003 at these norms) that it cannot pass
    the Lowe test, i.e. that it is dead on every route; the same margin bounds the live rows of image 0 from above by F.  With one
    block per live column the masks hold bit 1 only:
        sweep2_descriptor_pairs  <=  ceil512(F) x 600  +  ceil512(C) x 512.
    (Without the cap a column's mask reaches its second neighbour, an unrelated row in any block: up to ceil512(C) x 1100.)"""
    n1, ratio, margin = 1100, 0.8, 0.03
    imgs, planted = plant_job(n1, "float", n_planted=256, one_block=1)      # (480 planted rows: block 1 holds them all)
    assert all(p == 1 for x in planted for _, p in x["rows"])
    pairs = np.array([[0, 1]], np.int32)
    A, B = imgs
    _, fd0, _, fd1 = oracle.knn2(A, B)
    _, rd0, _, rd1 = oracle.knn2(B, A)
    maybe_live = lambda d0, d1: (d0 - margin) < ratio * (d1 + margin)
    C = len(planted)
    cols = np.zeros(N2, bool)
    cols[[p["col"] for p in planted]] = True
    assert not maybe_live(rd0[~cols], rd1[~cols]).any()          # unrelated columns are dead by a margin
    F = int(maybe_live(fd0, fd1).sum())
    assert F <= BLOCK                                               # (the planted rows, all in one block)
    c512 = lambda n: (n + BLOCK - 1) // BLOCK * BLOCK
    bound = c512(F) * N2 + c512(C) * BLOCK
    monkeypatch.setenv("MSFM_Q8", "2")
    monkeypatch.setenv("MSFM_Q8_DIRECT", "0" if route == "refined" else "1")
    with _lib.Context(0) as ctx:
        ctx.set_prefilter(2 if route == "fp16" else 1)
        for k, x in enumerate(imgs):
            ctx.upload_image(k, x)
        for cc in (True, False):
            got = ctx.match_pairs(pairs, ratio=ratio, cross_check=cc, max_distance=0.7)
            prof = ctx.profile()
            assert_route(prof, route, ratio, 1)
            assert same(got, oracle_lists(oracle, imgs, pairs, ratio, cc, 0.7)), (route, cc)
            print("sweep2_descriptor_pairs %d, bound %d (uncapped masks: up to %d)" % (prof["sweep2_descriptor_pairs"], bound,
                                                                                       c512(F) * N2 + c512(C) * n1))
            assert 0 < prof["sweep2_descriptor_pairs"] <= bound, (route, prof["sweep2_descriptor_pairs"], bound)
