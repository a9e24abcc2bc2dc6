// msfm_align.h -- map alignment arithmetic shared by the device kernels (msfm_align.hip.h, hipcc) and the host twins (host/HostTestApi.cpp,
// EstimateAlignment / TransformMap, g++): a robust similarity from the map's camera centres to known camera positions, and the edit that
// moves the whole map -- every pose and every point -- by a similarity.  A map lives in the gauge of its initial
// pair; the positions of a rig, an INS or an earlier reconstruction fix the frame the caller wants it in.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits; a NaN fails every decision.  onesided_jacobi and decompose's compare-and-swap network are
// msfm_pose.h's, centre and prepare_pose msfm_triangulate.h's, sample3 msfm_register.h's, mix64 / replay_adaptive msfm_fmat.h's,
// point_verdict msfm_refine.h's, succeeded msfm_refine_poses.h's, kKeptBits msfm_refine_camera.h's.
//
//   similarity      (s, Q, d): world' = s Q X + d, s > 0, Q row-major and a proper rotation (msfm_similarity).
//   prior           a pair (C, p): C the camera centre of a posed image (msfm_tri::centre of the session's pose), p the caller's position
//                   of it.  The m usable priors are the listed images with a valid pose, in list order.
//   sums            over a SET of priors, every sum in the order msfm_pose.h states for its statistics: partial l (l < 256) adds the
//                   set's members at the list positions l, l + 256, l + 512, .. in that order from 0.0 (positions outside the set are
//                   passed over); then the tree  for (s = 128; s >= 1; s /= 2) v[l] = v[l] + v[l + s], l < s;  the sum is v[0].
//                   A three-element sample is summed in the order idx[0], idx[1], idx[2] from 0.0.
//   fit             Umeyama 1991.  First the sums of C, of p and of 1.0 (the set's size n): the means mc, mp = sum / n.  Then the nine
//                   sums M[i][j] = sum (p - mp)[i] (C - mc)[j] and va = sum |C - mc|^2 (the squares added in index order).
//                   onesided_jacobi<3, 3> on the columns of M (M V = U S), columns ordered by norm with decompose's network; sigma_j
//                   the norms; u1, u2 the two largest columns normalised, u3 = u1 x u2, v3 = v1 x v2;
//                       Q = (u1 v1^T + u2 v2^T) + u3 v3^T      (proper by construction: the reflection case is covered)
//                       s = ((sigma0 + sigma1) + g sigma2) / va
//                       d = mp - s Q mc
//                   g = +1 iff (a3 . u3) (w3 . v3) >= 0, else -1, with a3 the rotated third column of M and w3 the third column of V:
//                   the two inner products carry the signs of det U and det V.  The rotations leave det V = +1, but every swap of
//                   the network exchanges a column of U and of V at once and flips BOTH signs, so (a3 . u3) alone is the sign of
//                   det U det V only after an even number of swaps.
//   valid           every number finite, va > 0, s > 0 and sigma1 > kMinSpread sigma0: centres on a line (a straight flight strip)
//                   leave the rotation about that line free.  kMinSpread is a definition, like kLambda0, not a measurement.
//   error           e = |p - (s Q C + d)|; a prior is an inlier iff e <= max_error (false for a NaN), in the prior's units.
//   robust          hypothesis `it` = the fit of the three priors sample3(mix64(kAlnSeed), it, m); an invalid sample counts 0, any
//                   other its inliers among all m.  Stopping: msfm_fmat::replay_adaptive<3> over the counts, scored in rounds of
//                   kAlnRound = 256 hypotheses: the result equals scoring all max_hypotheses; `hypotheses` = the hypotheses the rule
//                   evaluates before it stops (what a sequential loop would have fitted: three priors that all agree give 1), not
//                   the whole rounds that were scored.  The winner: the largest count, the lowest `it` among equals (MODEL).  No
//                   winner, or fewer than max(3, min_inliers) inliers: the estimate fails.
//   refits          at most kRefits = 4, the rule of MSFM_REG_REFINED repeated: the fit over the current model's inlier set STANDS iff
//                   it is valid and has at least as many inliers among all m; stop at the first refit that does not stand, and after
//                   one that stands with an unchanged inlier set (the next would repeat it).
//   least squares   max_hypotheses == 0: one fit of all m priors; every one is reported as an inlier and max_error is not read.
//   result          rms = sqrt(the inliers' e^2, summed in the order above, / n_inliers); per prior USED | INLIER and e.
//   transform       a valid pose becomes R' = R Q^T, t' = s t - R' d: the camera frame is scaled by s, so depths scale by s and no
//                   projection changes.  R is not re-orthogonalised, as everywhere.  A record with ATTEMPTED | POINT gets
//                   X' = s (Q X) + d and is evaluated again at X' under the new poses by msfm_ref::point_verdict with the session's
//                   camera and thresholds -- what msfm_rc::recalibrate_track does: residual slots of the used observations,
//                   mean_residual, tri_angle and the three verdict bits are rewritten, n_views and the inlier bytes are kept;
//                   status = ATTEMPTED | POINT | the three bits | (old & msfm_rc::kKeptBits) | MSFM_TRI_ALIGNED.  A non-finite X' (an
//                   overflow) gives ATTEMPTED | the kept bits | ALIGNED with every other field 0 and every residual slot -1.0, the
//                   shape the filter gives a removed point.  Under the identity 1 * (I X) + 0 and R I^T are exact: every X and every
//                   pose keeps its bits (but a zero's sign: -0.0 + 0.0 is +0.0).
#pragma once

#include "msfm_refine_camera.h"
#include "msfm_register.h"

#if !defined(__HIP_DEVICE_COMPILE__)   // (the host twins below)
#include <algorithm>
#include <vector>
#endif

namespace msfm_aln {

constexpr int kAlnRound = 256;          // hypotheses per round = partial sums = threads of aln_estimate_kernel
constexpr int kAlnTile = 256;           // priors per LDS tile of the scoring loop (12 KiB)
constexpr int kRefits = 4;
constexpr int kMaxHypotheses = 4096;
constexpr double kMinSpread = 1e-6;     // valid iff sigma1 > kMinSpread * sigma0
constexpr double kOrthoTol = 1e-9;      // msfm_transform_map: max |Q Q^T - I|
constexpr unsigned long long kAlnSeed = 0x4d6170416c69676eULL;

struct Prior {   // 48 bytes
    double C[3], p[3];
};

struct Params {
    double max_error, confidence;
    int32_t max_hypotheses, min_inliers;
};

struct Tally {
    int32_t transformed, lost, gained;
};

MSFM_FHD unsigned long long aln_seed() { return msfm_fmat::mix64(kAlnSeed); }

MSFM_FHD void clear_similarity(msfm_similarity* g) {
    g->s = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) g->Q[k] = 0.0;
    g->d[0] = g->d[1] = g->d[2] = 0.0;
}

// the record of an estimate that has not (or not yet) succeeded: n_listed and estimate_ms are the caller's
MSFM_FHD void clear_alignment(msfm_alignment* a, int n_used) {
    a->status = 0;
    a->n_listed = 0;
    a->n_used = n_used;
    a->n_inliers = 0;
    a->hypotheses = 0;
    a->refits = 0;
    clear_similarity(&a->similarity);
    a->rms = 0.0;
    a->estimate_ms = 0.0;
}

// e = |p - (s Q C + d)|
MSFM_FHD double prior_error(const msfm_similarity& g, const Prior& q) {
    double r[3];
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double y = g.s * (g.Q[3 * i] * q.C[0] + g.Q[3 * i + 1] * q.C[1] + g.Q[3 * i + 2] * q.C[2]) + g.d[i];
        r[i] = q.p[i] - y;
    }
    return sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
}

// what one prior adds to the first pass (C, p, 1.0) and to the second (M row-major, va)
MSFM_FHD void first_term(const Prior& q, double v[7]) {
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        v[i] = q.C[i];
        v[3 + i] = q.p[i];
    }
    v[6] = 1.0;
}
MSFM_FHD void second_term(const Prior& q, const double mc[3], const double mp[3], double v[10]) {
    const double c0 = q.C[0] - mc[0], c1 = q.C[1] - mc[1], c2 = q.C[2] - mc[2];
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double pi = q.p[i] - mp[i];
        v[3 * i] = pi * c0;
        v[3 * i + 1] = pi * c1;
        v[3 * i + 2] = pi * c2;
    }
    v[9] = c0 * c0 + c1 * c1 + c2 * c2;
}

// (s, Q, d) from the means and the ten sums of the second pass.  False: not valid (g is then not to be used).
MSFM_FHD bool fit_from_sums(const double mc[3], const double mp[3], const double acc[10], msfm_similarity* g) {
    double a[3][3], v[3][3], n[3];
MSFM_UNROLL
    for (int j = 0; j < 3; ++j)
MSFM_UNROLL
        for (int i = 0; i < 3; ++i) a[j][i] = acc[3 * i + j];   // a[j]: column j of M
    const double va = acc[9];
    msfm_pose::onesided_jacobi<3, 3>(a, v);
MSFM_UNROLL
    for (int j = 0; j < 3; ++j) n[j] = a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2];
    // descending by norm: compare-and-swap (0,1) (1,2) (0,1), whole columns, no runtime indexing
MSFM_UNROLL
    for (int step = 0; step < 3; ++step) {
        const int p = step == 1 ? 1 : 0, q = p + 1;
        const bool sw = n[q] > n[p];
        const double np = n[p], nq = n[q];
        n[p] = sw ? nq : np;
        n[q] = sw ? np : nq;
MSFM_UNROLL
        for (int k = 0; k < 3; ++k) {
            const double ap = a[p][k], aq = a[q][k], vp = v[p][k], vq = v[q][k];
            a[p][k] = sw ? aq : ap;
            a[q][k] = sw ? ap : aq;
            v[p][k] = sw ? vq : vp;
            v[q][k] = sw ? vp : vq;
        }
    }
    if (!(n[1] > 0.0) || !msfm_pose::finite(n[0])) return false;
    const double sg0 = sqrt(n[0]), sg1 = sqrt(n[1]), sg2 = sqrt(n[2]);
    if (!(sg1 > kMinSpread * sg0)) return false;
    const double i0 = 1.0 / sg0, i1 = 1.0 / sg1;
    const double u1[3] = {a[0][0] * i0, a[0][1] * i0, a[0][2] * i0}, u2[3] = {a[1][0] * i1, a[1][1] * i1, a[1][2] * i1};
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double* v1 = v[0];
    const double* v2 = v[1];
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    const double du = a[2][0] * u3[0] + a[2][1] * u3[1] + a[2][2] * u3[2];
    const double dv = v[2][0] * v3[0] + v[2][1] * v3[1] + v[2][2] * v3[2];
    const double sign = du * dv >= 0.0 ? 1.0 : -1.0;
    bool ok = true;
MSFM_UNROLL
    for (int i = 0; i < 3; ++i)
MSFM_UNROLL
        for (int j = 0; j < 3; ++j) {
            g->Q[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
            ok = ok && msfm_pose::finite(g->Q[3 * i + j]);
        }
    g->s = ((sg0 + sg1) + sign * sg2) / va;
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        g->d[i] = mp[i] - g->s * (g->Q[3 * i] * mc[0] + g->Q[3 * i + 1] * mc[1] + g->Q[3 * i + 2] * mc[2]);
        ok = ok && msfm_pose::finite(g->d[i]);
    }
    return ok && msfm_pose::finite(g->s) && va > 0.0 && g->s > 0.0;
}

// the fit of a three-element sample, summed in the order q0, q1, q2 from 0.0
MSFM_FHD bool fit_sample(const Prior& q0, const Prior& q1, const Prior& q2, msfm_similarity* g) {
    double f0[7], f1[7], f2[7], mc[3], mp[3];
    first_term(q0, f0);
    first_term(q1, f1);
    first_term(q2, f2);
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        mc[i] = (((0.0 + f0[i]) + f1[i]) + f2[i]) / 3.0;
        mp[i] = (((0.0 + f0[3 + i]) + f1[3 + i]) + f2[3 + i]) / 3.0;
    }
    double s0[10], s1[10], s2[10], acc[10];
    second_term(q0, mc, mp, s0);
    second_term(q1, mc, mp, s1);
    second_term(q2, mc, mp, s2);
MSFM_UNROLL
    for (int k = 0; k < 10; ++k) acc[k] = ((0.0 + s0[k]) + s1[k]) + s2[k];
    return fit_from_sums(mc, mp, acc, g);
}

// hypothesis `it` over the m priors read through prior(k)
template <class F>
MSFM_FHD bool hypothesis(F prior, int m, unsigned long long seed, int it, msfm_similarity* g) {
    int idx[3];
    msfm_reg::sample3(seed, it, m, idx);
    const Prior q0 = prior(idx[0]), q1 = prior(idx[1]), q2 = prior(idx[2]);
    return fit_sample(q0, q1, q2, g);
}

// The fit over the set {k : in(prior k)} through the reduced passes of `pv` (see estimate).  False: not valid.
template <class P, class S>
MSFM_FHD bool fit_set(const P& pv, S in, msfm_similarity* g) {
    double a7[7], a10[10], mc[3], mp[3];
    pv.template sum<7>([&](int k, double* v) {
        const Prior q = pv.prior(k);
        if (!in(q)) return false;
        first_term(q, v);
        return true;
    }, a7);
    if (!(a7[6] >= 3.0)) return false;
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
        mc[i] = a7[i] / a7[6];
        mp[i] = a7[3 + i] / a7[6];
    }
    pv.template sum<10>([&](int k, double* v) {
        const Prior q = pv.prior(k);
        if (!in(q)) return false;
        second_term(q, mc, mp, v);
        return true;
    }, a10);
    return fit_from_sums(mc, mp, a10, g);
}

// The whole estimate.  `pv` owns the m priors and gives the REDUCED passes, the same bits wherever it runs (on the device every thread
// of the one workgroup calls every member, and every thread holds the same result: the control flow is uniform):
//   pv.m()                       the number of usable priors
//   pv.prior(k)                  prior k
//   pv.sum<K>(term, out)         term(k, v) -> bool: prior k is in the set and v[0 .. K) is what it adds; out: the K sums in the order of
//                                the header's summation paragraph.  term is called exactly once for every k < m.
//   pv.count(term, out)          term(k, c): integer adds into c[0], c[1]; out: the two totals
//   pv.score(round, seed, prm)   the counts of the hypotheses 256 round .. 256 round + 255 (those below max_hypotheses)
//   pv.count_at(it)              the count of a scored hypothesis
//   pv.store(k, flags, error)    the per-prior record of prior k
// out: everything but n_listed and estimate_ms.
template <class P>
MSFM_FHD void estimate(const P& pv, const Params& prm, msfm_alignment* out) {
    const int m = pv.m();
    msfm_alignment a;
    clear_alignment(&a, m);
    const bool ls = prm.max_hypotheses == 0;
    msfm_similarity cur;
    clear_similarity(&cur);
    bool have = false;
    int count = 0;
    if (m >= 3) {
        a.status = MSFM_ALN_ATTEMPTED | (ls ? MSFM_ALN_LEAST_SQUARES : 0);
        if (ls) {
            have = fit_set(pv, [](const Prior&) { return true; }, &cur);
            count = have ? m : 0;
        } else {
            const unsigned long long seed = aln_seed();
            int best_it = -1, best = 0, read = 0;
            for (int r = 1; r <= kMaxHypotheses / kAlnRound; ++r) {
                pv.score(r - 1, seed, prm);
                const int avail = r * kAlnRound < prm.max_hypotheses ? r * kAlnRound : prm.max_hypotheses;
                bool decided = false;
                read = 0;
                best_it = msfm_fmat::replay_adaptive<3>(m, prm.max_hypotheses, prm.confidence, [&](int it) {
                    read += 1;
                    return pv.count_at(it);
                }, &best, avail, &decided);
                if (decided) break;
            }
            a.hypotheses = read;   // (the counts the decided rule read: 0 .. read - 1)
            if (best_it >= 0) {
                have = hypothesis([&](int k) { return pv.prior(k); }, m, seed, best_it, &cur);   // (valid: it counted inliers)
                count = have ? best : 0;
            }
        }
    }
    if (have) a.status |= MSFM_ALN_MODEL;
    const int need = prm.min_inliers > 3 ? prm.min_inliers : 3;
    a.n_inliers = count;
    if (!have || count < need) {
        int all[2];
        pv.count([&](int k, int* c) {
            pv.store(k, MSFM_ALN_USED, -1.0);
            c[0] += 1;
        }, all);
        *out = a;
        return;
    }
    if (!ls) {
        for (int r = 0; r < kRefits; ++r) {
            msfm_similarity nw;
            const msfm_similarity held = cur;
            if (!fit_set(pv, [&](const Prior& q) { return prior_error(held, q) <= prm.max_error; }, &nw)) break;
            int c2[2];
            pv.count([&](int k, int* c) {
                const Prior q = pv.prior(k);
                const bool now = prior_error(nw, q) <= prm.max_error, was = prior_error(held, q) <= prm.max_error;
                c[0] += now ? 1 : 0;
                c[1] += now != was ? 1 : 0;
            }, c2);
            if (c2[0] < count) break;
            cur = nw;
            count = c2[0];
            a.refits += 1;
            a.status |= MSFM_ALN_REFIT;
            if (c2[1] == 0) break;
        }
    }
    double ss[1];
    pv.template sum<1>([&](int k, double* v) {
        const double e = prior_error(cur, pv.prior(k));
        const bool in = ls || e <= prm.max_error;
        pv.store(k, MSFM_ALN_USED | (in ? MSFM_ALN_INLIER : 0), msfm_pose::canonical(e));
        v[0] = e * e;
        return in;
    }, ss);
    a.status |= MSFM_ALN_SUCCEEDED;
    a.n_inliers = count;
    a.similarity = cur;
    a.rms = sqrt(ss[0] / (double)count);
    *out = a;
}

// ---- the transform --------------------------------------------------------------------------------------------------------------------
// what msfm_transform_map accepts: s finite and positive, d finite, max |Q Q^T - I| <= kOrthoTol, det Q > 0
MSFM_FHD bool similarity_ok(const msfm_similarity& g) {
    bool ok = msfm_pose::finite(g.s) && g.s > 0.0 && msfm_pose::finite(g.d[0]) && msfm_pose::finite(g.d[1]) && msfm_pose::finite(g.d[2]);
MSFM_UNROLL
    for (int i = 0; i < 3; ++i)
MSFM_UNROLL
        for (int j = 0; j < 3; ++j) {
            const double e = (g.Q[3 * i] * g.Q[3 * j] + g.Q[3 * i + 1] * g.Q[3 * j + 1] + g.Q[3 * i + 2] * g.Q[3 * j + 2]) - (i == j ? 1.0 : 0.0);
            ok = ok && e <= kOrthoTol && e >= -kOrthoTol;   // (false for a NaN)
        }
    const double det = g.Q[0] * (g.Q[4] * g.Q[8] - g.Q[5] * g.Q[7]) - g.Q[1] * (g.Q[3] * g.Q[8] - g.Q[5] * g.Q[6]) +
                       g.Q[2] * (g.Q[3] * g.Q[7] - g.Q[4] * g.Q[6]);
    return ok && det > 0.0;
}

// R' = R Q^T, t' = s t - R' d.  False: the new pose is not finite.
MSFM_FHD bool transform_pose(const msfm_similarity& g, const double R[9], const double t[3], double Rn[9], double tn[3]) {
    bool ok = true;
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) {
MSFM_UNROLL
        for (int j = 0; j < 3; ++j) {
            Rn[3 * i + j] = R[3 * i] * g.Q[3 * j] + R[3 * i + 1] * g.Q[3 * j + 1] + R[3 * i + 2] * g.Q[3 * j + 2];
            ok = ok && msfm_pose::finite(Rn[3 * i + j]);
        }
        tn[i] = g.s * t[i] - (Rn[3 * i] * g.d[0] + Rn[3 * i + 1] * g.d[1] + Rn[3 * i + 2] * g.d[2]);
        ok = ok && msfm_pose::finite(tn[i]);
    }
    return ok;
}

// X' = s (Q X) + d
MSFM_FHD void transform_point(const msfm_similarity& g, const double X[3], double Xn[3]) {
MSFM_UNROLL
    for (int i = 0; i < 3; ++i) Xn[i] = g.s * (g.Q[3 * i] * X[0] + g.Q[3 * i + 1] * X[1] + g.Q[3 * i + 2] * X[2]) + g.d[i];
}

// One track with ATTEMPTED | POINT after the poses changed: obs: its n Obs (their ranks index `poses`, the NEW table), residuals: its n
// element-aligned slots; rec: read and rewritten.
MSFM_FHD void align_track(const msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, double f, const msfm_ref::Verdict& vd,
                          const msfm_similarity& g, msfm_point3d* rec, double* residuals, Tally* tally) {
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    double Xn[3];
    transform_point(g, X, Xn);
    msfm_point3d r = old;
    if (msfm_pose::finite(Xn[0]) && msfm_pose::finite(Xn[1]) && msfm_pose::finite(Xn[2])) {
        msfm_ref::PointVerdict v;
        msfm_ref::point_verdict(obs, n, poses, f, vd, Xn, residuals, &v);
        r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits | (old.status & msfm_rc::kKeptBits) | MSFM_TRI_ALIGNED;
        r.X[0] = Xn[0];
        r.X[1] = Xn[1];
        r.X[2] = Xn[2];
        r.mean_residual = msfm_pose::canonical(v.sum / (double)v.count);   // (THE NaN RULE: a huge X' can make an error NaN)
        r.tri_angle = v.angle;
    } else {
        msfm_tri::clear_point(&r);
        r.status = MSFM_TRI_ATTEMPTED | (old.status & msfm_rc::kKeptBits) | MSFM_TRI_ALIGNED;
        for (int k = 0; k < n; ++k) residuals[k] = -1.0;
    }
    *rec = r;
    tally->transformed = 1;
    tally->lost = (msfm_rp::succeeded(old) && !msfm_rp::succeeded(r)) ? 1 : 0;
    tally->gained = (!msfm_rp::succeeded(old) && msfm_rp::succeeded(r)) ? 1 : 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twins -------------------------------------------------------------------------------------------------------------------
// the reduced passes of estimate on the host, literally the header's summation paragraph
struct HostPriors {
    const Prior* priors;
    int n;
    int* counts;                       // kMaxHypotheses
    msfm_alignment_residual* records;  // n
    int m() const { return n; }
    Prior prior(int k) const { return priors[k]; }
    template <int K, class F>
    void sum(F term, double out[K]) const {
        std::vector<double> part((size_t)kAlnRound * K, 0.0);
        for (int l = 0; l < kAlnRound; ++l)
            for (int k = l; k < n; k += kAlnRound) {
                double v[K];
                if (!term(k, v)) continue;
                for (int j = 0; j < K; ++j) part[(size_t)j * kAlnRound + l] = part[(size_t)j * kAlnRound + l] + v[j];
            }
        for (int s = kAlnRound / 2; s >= 1; s /= 2)
            for (int l = 0; l < s; ++l)
                for (int j = 0; j < K; ++j) part[(size_t)j * kAlnRound + l] = part[(size_t)j * kAlnRound + l] + part[(size_t)j * kAlnRound + l + s];
        for (int j = 0; j < K; ++j) out[j] = part[(size_t)j * kAlnRound];
    }
    template <class F>
    void count(F term, int* out) const {
        int c[2] = {0, 0};
        for (int k = 0; k < n; ++k) term(k, c);
        out[0] = c[0];
        out[1] = c[1];
    }
    void score(int round, unsigned long long seed, const Params& prm) const {
        for (int it = round * kAlnRound; it < (round + 1) * kAlnRound && it < prm.max_hypotheses; ++it) {
            msfm_similarity g;
            int c = 0;
            if (hypothesis([&](int k) { return priors[k]; }, n, seed, it, &g))
                for (int k = 0; k < n; ++k) c += prior_error(g, priors[k]) <= prm.max_error ? 1 : 0;
            counts[it] = c;
        }
    }
    int count_at(int it) const { return counts[it]; }
    void store(int k, int flags, double error) const { records[k] = msfm_alignment_residual{flags, 0, error}; }
};

// The m usable priors in list order -> the record (but n_listed and estimate_ms) and the m per-prior records.
inline void EstimateAlignment(const Prior* priors, int m, const Params& prm, msfm_alignment* out, msfm_alignment_residual* records) {
    std::vector<int> counts((size_t)kMaxHypotheses, 0);
    const HostPriors pv{priors, m, counts.data(), records};
    estimate(pv, prm, out);
}

struct TransformCounts {
    long long poses_transformed, points_transformed, points_lost, points_gained, succeeded;
};

// The session's pose list moved by g: false (nothing written) when a new pose is not finite.  Entries without a valid pose are kept.
inline bool TransformPoses(const msfm_similarity& g, const msfm_pose_rt* in, int n, msfm_pose_rt* out, long long* moved) {
    std::vector<msfm_pose_rt> np(in, in + n);
    long long c = 0;
    for (int k = 0; k < n; ++k) {
        msfm_tri::Pose p;
        msfm_tri::prepare_pose(in[k], &p);
        if (!p.valid) continue;
        if (!transform_pose(g, in[k].R, in[k].t, np[(size_t)k].R, np[(size_t)k].t)) return false;
        c += 1;
    }
    std::copy(np.begin(), np.end(), out);
    *moved = c;
    return true;
}

// tracks, rank_of_id, kxy, mask as RefineCamera takes them (all tracks); poses: the table of the NEW poses; points / residuals: read and
// rewritten.  counts: the four point counters are filled (poses_transformed is the caller's).
inline void TransformMap(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, int64_t n_tracks, const int* rank_of_id,
                         const float* const* kxy, const msfm_tri::Pose* poses, const uint8_t* mask, const msfm_emat::Camera& cam,
                         const msfm_ref::Verdict& vd, const msfm_similarity& g, msfm_point3d* points, double* residuals,
                         TransformCounts* counts) {
    const double f = (cam.fx + cam.fy) / 2.0;
    std::vector<msfm_ref::Obs> obs;
    counts->points_transformed = counts->points_lost = counts->points_gained = counts->succeeded = 0;
    for (int64_t t = 0; t < n_tracks; ++t) {
        if (msfm_ref::eligible(points[t])) {
            const int64_t b = offsets[t];
            const int n = (int)(offsets[t + 1] - b);
            const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
            obs.resize((size_t)std::max(n, 1));
            msfm_ref::host_obs(a, n, mask ? mask + b : nullptr, cam, obs.data());
            Tally tl;
            align_track(obs.data(), n, poses, f, vd, g, points + t, residuals + b, &tl);
            counts->points_transformed += tl.transformed;
            counts->points_lost += tl.lost;
            counts->points_gained += tl.gained;
        }
        counts->succeeded += msfm_rp::succeeded(points[t]) ? 1 : 0;
    }
}
#endif

}  // namespace msfm_aln
