"""The ratio cap of the reverse thresholds (monocularsfm_amd/csrc/msfm_hostutil.h: msfm_ratio_cap_distance, msfm_ratio_cap_sweep,
msfm_ratio_cap_sweep_i8) and the d1 = +inf branch of the order certificate (msfm_order_sensitive), compiled here with g++ and driven
against an fp64 statement of what they promise.

The invariant.  With e = kOrderEps, an element t != best VIOLATES a column's Lowe test when its pinned fp32 distance has
d0 (1 + e) >= ratio d_t (1 - e).  Every violator must lie within the capped threshold -- S~_t <= T in the sweeps' space, a real
distance <= the capped bound on route Q -- and so must the best element.  The driver takes the WORST values consistent with what the
kernels know (the best element's exact S at the top of its interval, the violator's at the bottom of its own) and checks

  * random (s0, norms, ratio) and ratio in {0.05, 0.6, 0.8, 0.95}, s0 = 0 and below, equal best and second;
  * an element exactly at the cap and one ulp below it is admitted by the sweep's test (S~ <= T); the element one ulp ABOVE the cap,
    which the sweep drops, cannot violate whatever its exact value is;
  * the integer branch for both parities of the query norm and of the candidates' norms (S~ = S - parity bits), every value exact;
  * the certificate: candidates = every violator + a random subset of the rest; the decision and the certificate computed from
    (d0, smallest candidate or +inf) equal those computed from (d0, true second neighbour), forward and reverse, with the distance
    cut on either side of d0.
The reference's test is FeatureUtils::FilterMatches' m[0].distance < ratio * m[1].distance
(/root/reference/src/Feature/FeatureUtils.cpp:150-156)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "monocularsfm_amd", "csrc")

DRIVER = r"""
#include "msfm_hostutil.h"
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

static const double E = kOrderEps;
static const double G = 4.0e-6;            // pinned fp32 order vs real arithmetic, relative, on a distance (msfm_kernels.hip.h)
static const float RATIOS[] = {0.05f, 0.6f, 0.8f, 0.95f};

static bool violates(double d0, double dt, float ratio) { return d0 * (1.0 + E) >= (double)ratio * (dt * (1.0 - E)); }
static float up(float x) { return std::nextafterf(x, INFINITY); }
static float down(float x) { return std::nextafterf(x, -INFINITY); }

int main() {
    std::mt19937_64 rng(20260);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long long checked = 0;

    // ---- S~ space, fp16 sweep ------------------------------------------------------------------------------------------
    for (int trial = 0; trial < 400000; ++trial) {
        const float ratio = trial % 3 ? RATIOS[trial % 4] : (float)(0.05 + 0.9 * U(rng));
        const float norms = (float)std::pow(10.0, -2.0 + 5.0 * U(rng));
        const float eps = 1.5e-3f * norms + 1.0e-6f * 2.f * std::sqrt(norms);
        float s0;
        switch (trial % 7) {
            case 0: s0 = 0.f; break;
            case 1: s0 = -eps; break;                       // S~ may undershoot an exact 0 by eps
            case 2: s0 = eps * (float)U(rng); break;
            default: s0 = norms * (float)(2.0 * U(rng) * U(rng)); break;
        }
        const float cap = msfm_ratio_cap_sweep(s0, eps, norms, ratio);
        if (!(cap >= s0)) { std::printf("sweep: best beyond the cap (s0 %g cap %g)\n", s0, cap); return 1; }
        // equal best and second: both within eps of one exact S, so the second's S~ <= s0 + 2 eps
        if (!((double)cap >= (double)s0 + 2.0 * (double)eps)) { std::printf("sweep: a tie of the best beyond the cap\n"); return 1; }
        // the worst case: the best element's exact S at the top of its interval; the largest violator; its S~ at the top of its own
        const double S0 = std::fmax((double)s0 + (double)eps, 0.0);
        const double q = (1.0 + E) / ((double)ratio * (1.0 - E));
        const double St = S0 * q * q * (1.0 + 4.0 * 5.97e-8);   // (d = sqrtf(S): two roundings each side)
        if (!((double)cap >= St + (double)eps)) { std::printf("sweep: violator beyond the cap: s0 %g eps %g ratio %g cap %g need %.9g\n", s0, eps, ratio, cap, St + eps); return 1; }
        // at the cap and one ulp below: admitted (the sweep's test is S~ <= T); one ulp above: dropped -- it must not violate
        const float T = cap;
        if (!(cap <= T) || !(down(cap) <= T) || (up(cap) <= T)) { std::printf("sweep: admission at the cap\n"); return 1; }
        const double St_min = (double)up(cap) - (double)eps;   // the smallest exact S of a dropped element
        const float d0 = std::sqrt((float)S0), dt = std::sqrt((float)std::fmax(St_min, 0.0));
        if (violates((double)up(d0), (double)down(dt), ratio)) { std::printf("sweep: the element above the cap violates (ratio %g)\n", ratio); return 1; }
        ++checked;
    }

    // ---- distance space, route Q ---------------------------------------------------------------------------------------
    for (int trial = 0; trial < 400000; ++trial) {
        const float ratio = trial % 3 ? RATIOS[trial % 4] : (float)(0.05 + 0.9 * U(rng));
        const float u0 = trial % 11 == 0 ? 0.f : (float)(2.0 * U(rng) * U(rng));
        const float u1 = trial % 5 == 0 ? u0 : u0 + (float)(2.0 * U(rng));   // (equal best and second: u1 == u0)
        const float uc = msfm_ratio_cap_distance(u0, u1, ratio);
        if (uc > u1) { std::printf("distance: cap above u1\n"); return 1; }
        if (uc == u1) { ++checked; continue; }               // today's bound: nothing new to prove
        // the best element: pinned d0 <= u0 (1 + g), real <= that / (1 - g)
        const double d0 = (double)u0 * (1.0 + G);
        if (!((double)uc >= d0 / (1.0 - G))) { std::printf("distance: best beyond the cap\n"); return 1; }
        const double dt = d0 * (1.0 + E) / ((double)ratio * (1.0 - E));   // the largest violator, pinned
        if (!((double)uc >= dt / (1.0 - G))) { std::printf("distance: violator beyond the cap (u0 %g ratio %g)\n", u0, ratio); return 1; }
        // a real distance one ulp above the cap: pinned >= real (1 - g) -- not a violator
        if (u0 > 0.f && violates(d0, (double)up(uc) * (1.0 - G), ratio)) { std::printf("distance: the element above the cap violates\n"); return 1; }
        ++checked;
    }

    // ---- integer sweeps: S~ = S - (n'_q & 1) - (n'_t & 1), n'_t = n'_q + S mod 2 --------------------------------------------
    for (float ratio : RATIOS)
        for (int pq = 0; pq < 2; ++pq)            // parity of the query norm (odd and even)
            for (int S0 = 0; S0 < 1500; S0 += (S0 < 64 ? 1 : 7)) {
                // the column's smallest S~: the best element's own, or a further element's that undershoots it (>= S0 - 2)
                for (int s0 = S0 - 2; s0 <= S0 - pq - ((pq + S0) & 1); ++s0) {
                    const float cap = msfm_ratio_cap_sweep_i8((float)s0, 2.f, ratio);
                    if (cap != std::floor(cap)) { std::printf("i8: cap not an integer\n"); return 1; }
                    if (!(cap >= (float)S0)) { std::printf("i8: best beyond the cap\n"); return 1; }
                    const float d0 = std::sqrt((float)S0);
                    const int hi = (int)((S0 + 4) / ((double)ratio * ratio) * 1.01) + 8;
                    for (int St = S0; St <= hi; ++St) {    // (St == S0: equal best and second)
                        const float dt = std::sqrt((float)St);
                        const bool fails = !(d0 < ratio * dt);                       // the reference's fp32 test
                        const int st = St - pq - ((pq + St) & 1);                    // both parities of the candidate's norm occur
                        if ((fails || violates(d0, dt, ratio)) && !((float)st <= cap)) {
                            std::printf("i8: violator beyond the cap: S0 %d St %d ratio %g cap %g\n", S0, St, ratio, cap);
                            return 1;
                        }
                        ++checked;
                    }
                    // one past the cap: dropped, and whatever its parities (S >= S~) it passes the test
                    const float dn = std::sqrt(cap + 1.f);
                    if (!(d0 < ratio * dn) || violates(d0, dn, ratio)) { std::printf("i8: the element above the cap violates\n"); return 1; }
                }
            }

    // ---- the certificate: (d0, smallest candidate or +inf) against the brute-force (d0, true d1) -------------------------------
    long long inf_rows = 0, sens_rows = 0;
    for (int trial = 0; trial < 600000; ++trial) {
        const float ratio = RATIOS[trial % 4];
        const float d0 = trial % 13 == 0 ? 0.f : (float)(0.02 + U(rng));
        const int n = 1 + (int)(rng() % 6);
        std::vector<float> d(n);
        const double edge = (double)d0 / (double)ratio;
        for (int k = 0; k < n; ++k) {
            const int kind = (int)(rng() % 5);
            double v = kind == 0 ? edge * (1.0 + (U(rng) - 0.5) * 1.0e-4)                 // on the violation boundary
                     : kind == 1 ? (double)d0 * (1.0 + U(rng) * 3.0e-5)                   // next to the best (ties in sqrt space)
                     : kind == 2 ? (double)d0                                             // equal best and second
                                 : edge * (0.9 + 1.5 * U(rng));
            d[k] = (float)std::fmax(v, (double)d0);
        }
        float d1 = INFINITY, c1 = INFINITY;
        for (int k = 0; k < n; ++k) {
            d1 = std::fmin(d1, d[k]);
            const bool candidate = violates((double)d0, (double)d[k], ratio) || rng() % 3 == 0;   // every violator + strays
            if (candidate) c1 = std::fmin(c1, d[k]);
        }
        if (c1 == INFINITY) ++inf_rows;
        double cuts[] = {1e9, (double)d0, std::nextafter((double)d0, 0.0), std::nextafter((double)d0, 9.0), (double)d0 * (1.0 + 0.5e-5), 0.7};
        for (double md : cuts)
            for (int fwd = 0; fwd < 2; ++fwd) {
                const bool want = msfm_order_sensitive(3, d0, d1, ratio, md, fwd != 0);
                const bool got = msfm_order_sensitive(3, d0, c1, ratio, md, fwd != 0);
                const bool keep_want = d0 < ratio * d1, keep_got = c1 == INFINITY || d0 < ratio * c1;
                if (want != got || keep_want != keep_got) {
                    std::printf("certificate: d0 %.9g d1 %.9g capped d1 %.9g ratio %g cut %.17g fwd %d: %d/%d vs %d/%d\n", d0, d1, c1, ratio, md, fwd,
                                (int)got, (int)keep_got, (int)want, (int)keep_want);
                    return 1;
                }
                sens_rows += want;
                ++checked;
            }
    }
    // "fewer than two neighbours" stays what it was: no match, nothing to certify
    if (msfm_order_sensitive(3, 0.3f, kNoNeighbour, 0.8f, 0.7, true) || msfm_order_sensitive(-1, 0.3f, INFINITY, 0.8f, 0.7, true)) { std::printf("certificate: no neighbour\n"); return 1; }
    // +inf: certified unless the forward cut straddles d0
    if (msfm_order_sensitive(3, 0.3f, INFINITY, 0.8f, 0.7, true) || !msfm_order_sensitive(3, 0.7f, INFINITY, 0.8f, 0.7, true) ||
        msfm_order_sensitive(3, 0.7f, INFINITY, 0.8f, 0.7, false)) { std::printf("certificate: +inf\n"); return 1; }
    // the switch: match lists with 0 < ratio <= 0.9, always inside the compacted sweep 2 (the dense sweep keeps the uncapped thresholds)
    if (!msfm_ratio_cap_on(1, 0.05f) || !msfm_ratio_cap_on(1, 0.8f) || !msfm_ratio_cap_on(1, 0.9f) || msfm_ratio_cap_on(0, 0.8f) ||
        msfm_ratio_cap_on(1, 0.f) || msfm_ratio_cap_on(1, std::nextafterf(0.9f, 1.f)) || msfm_ratio_cap_on(1, 0.95f) ||
        msfm_ratio_cap_on(1, 1.f)) { std::printf("cap switch\n"); return 1; }
    for (float r : {0.3f, 0.8f, 0.9f, 0.95f, 0.96f, 1.0f, 0.f})
        for (int p = 0; p < 2; ++p)
            if (msfm_ratio_cap_on(p, r) && !msfm_compact_sweep2(p, r)) { std::printf("cap outside the compacted sweep\n"); return 1; }
    std::printf("ok %lld inf %lld sens %lld\n", checked, inf_rows, sens_rows);
    return 0;
}
"""


def test_ratio_cap_keeps_every_violator_and_the_certificate(tmp_path):
    src = tmp_path / "ratio_cap_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "ratio_cap_driver"
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    last = run.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000000
    assert int(last[3]) > 10000 and int(last[5]) > 10000      # both branches of the certificate were exercised
