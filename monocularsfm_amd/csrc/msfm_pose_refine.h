// msfm_pose_refine.h -- two-view pose refinement arithmetic shared by the device kernel (msfm_verify_pose_refine.hip.h, hipcc) and the
// host twin (host/GeometricVerification.cpp, RefineTwoView, g++): the relative pose of a valid two-view record is moved to the minimum
// of the Sampson error over the pair's kept matches by Levenberg-Marquardt, one 5 x 5 system per pair.  The
// Sampson error eliminates the points, so nothing is shared between pairs and no point is an unknown.  n_kept and the match lists never
// change.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  lm_minimise (the LM loop, its constants, STOP_*) is msfm_refine.h's, cayley_update
// msfm_register.h's, evaluate and finish_record msfm_pose.h's.
//
//   input           the valid record's (R, t) and the pair's kept list: the nE E-inliers, in list order, in the normalised undistorted
//                   coordinates the record was computed from.
//   eligible        the record is valid and n_kept >= min_matches.
//   residual        per kept match  r_i = f num / sqrt(den),  num and den those of msfm_emat::sampson under E = [t]x R,
//                   f = (fx + fy) / 2;  the cost c = sum r_i^2 is in px^2.
//   unknowns        a in R^3:  R <- C(a) R  with the Cayley map of msfm_reg::cayley_update (C(a) = I + 2 [a]x + O(a^2));
//                   b in R^2:  t <- (t + B b) / |t + B b|,  B = [b1 b2]:  e the unit axis of the smallest |t_k| (the lowest index among
//                   equal ones),  b1 = (t x e) / |t x e|,  b2 = t x b1  -- at the state the step starts from.  |t| = 1 and a proper R
//                   are kept by construction.
//   Jacobian        analytic:  dE/da_k = 2 [t]x [e_k]x R,  dE/db_j = [b_j]x R;  with a = E x1, b = E^T x2 and D one of the five:
//                   dnum = x2^T D x1,  hd = a0 (D x1)_0 + a1 (D x1)_1 + b0 (D^T x2)_0 + b1 (D^T x2)_1,  J = f (dnum - num hd / den) / sqrt(den).
//   sums            kSums = 21: the 15 of the upper triangle of J^T J (00 01 .. 04 11 .. 44), the 5 of J^T r, the cost -- in
//                   msfm_pose.h's STATED ORDER: partial l (l < kLanes = 256) adds the kept matches l, l + 256, .. from 0.0, then the tree
//                   part[l] = part[l] + part[l + s], l < s, for s = 128 .. 1; the sum is part[0].
//   step            (H + lambda diag H) delta = -g by a 5 x 5 Cholesky, delta = (a, b).  A pivot that is not > 0, a non-finite delta or a
//                   non-finite new state: the step is rejected without a cost evaluation.
//   LM              msfm_ref::lm_minimise over PairProblem: depth is always true, stop_scale is 1, d2 = |a|^2 + |b|^2.
//   standing        after the loop the record's statistics are computed again under the final pose exactly as tv_pose_kernel's steps 5
//                   and 6 do them (evaluate per kept match, the two sums in the stated order, the exact median, finish_record);
//                   n_positive_depth is the number of kept matches evaluate puts in front of both cameras (msfm_pose::in_front's test).
//                   The refined record replaces the old one iff a step was accepted and neither n_positive_depth nor n_triangulated is
//                   lower than before.  Otherwise not one byte of the record changes.
//   refinement      msfm_two_view_refinement: all zero for a pair that is not eligible; else status ELIGIBLE | STEP_ACCEPTED | REFINED,
//                   the loop's stop, steps, accepted, the two counts of the old record, cost_before, and cost_after = the final cost when
//                   the refined record stands, cost_before when it does not.
#pragma once

#include "msfm_pose.h"
#include "msfm_refine.h"
#include "msfm_register.h"

namespace msfm_tvr {

constexpr int kLanes = msfm_pose::kLanes;   // partial sums = threads of a tv_refine_kernel workgroup
constexpr int kSums = 21;                   // 15 of J^T J | 5 of J^T r | the cost
constexpr int kCostSum = 20;

struct State {
    double R[9], t[3];
};
struct System {
    double acc[kSums];
};

MSFM_FHD msfm_two_view_refine_params default_params() { return msfm_two_view_refine_params{10, 15, 1e-6}; }

// M = [t]x G (row-major)
MSFM_FHD void cross_mat(const double t[3], const double G[9], double M[9]) {
MSFM_UNROLL
    for (int c = 0; c < 3; ++c) {
        M[c] = t[1] * G[6 + c] - t[2] * G[3 + c];
        M[3 + c] = t[2] * G[c] - t[0] * G[6 + c];
        M[6 + c] = t[0] * G[3 + c] - t[1] * G[c];
    }
}

// b1 = B[0 .. 3), b2 = B[3 .. 6)
MSFM_FHD void tangent_basis(const double t[3], double B[6]) {
    const double m0 = t[0] >= 0.0 ? t[0] : -t[0], m1 = t[1] >= 0.0 ? t[1] : -t[1], m2 = t[2] >= 0.0 ? t[2] : -t[2];
    const bool k0 = m0 <= m1 && m0 <= m2, k1 = !k0 && m1 <= m2;
    // t x e for e = e0: (0, t2, -t1); e1: (-t2, 0, t0); e2: (t1, -t0, 0)
    const double c0 = k0 ? 0.0 : (k1 ? -t[2] : t[1]), c1 = k0 ? t[2] : (k1 ? 0.0 : -t[0]), c2 = k0 ? -t[1] : (k1 ? t[0] : 0.0);
    const double inv = 1.0 / sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    B[0] = c0 * inv;
    B[1] = c1 * inv;
    B[2] = c2 * inv;
    B[3] = t[1] * B[2] - t[2] * B[1];
    B[4] = t[2] * B[0] - t[0] * B[2];
    B[5] = t[0] * B[1] - t[1] * B[0];
}

// E = [t]x R and its five derivatives D[k] at (a, b) = 0
MSFM_FHD void linear_model(const State& s, double E[9], double D[5][9]) {
    cross_mat(s.t, s.R, E);
    const double* R = s.R;
    // [e_k]x R: e0 x v = (0, -v2, v1), e1 x v = (v2, 0, -v0), e2 x v = (-v1, v0, 0), column by column
    const double G0[9] = {0.0, 0.0, 0.0, -R[6], -R[7], -R[8], R[3], R[4], R[5]};
    const double G1[9] = {R[6], R[7], R[8], 0.0, 0.0, 0.0, -R[0], -R[1], -R[2]};
    const double G2[9] = {-R[3], -R[4], -R[5], R[0], R[1], R[2], 0.0, 0.0, 0.0};
    cross_mat(s.t, G0, D[0]);
    cross_mat(s.t, G1, D[1]);
    cross_mat(s.t, G2, D[2]);
MSFM_UNROLL
    for (int k = 0; k < 3; ++k)
MSFM_UNROLL
        for (int i = 0; i < 9; ++i) D[k][i] = 2.0 * D[k][i];
    double B[6];
    tangent_basis(s.t, B);
    cross_mat(B, R, D[3]);
    cross_mat(B + 3, R, D[4]);
}

// r of one kept match under E
MSFM_FHD double residual(const double E[9], double f, double x1, double y1, double x2, double y2) {
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double num = x2 * a0 + y2 * a1 + a2;
    return f * num / sqrt(a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// r and its five derivatives
MSFM_FHD double jacobian(const double E[9], const double D[5][9], double f, double x1, double y1, double x2, double y2, double J[5]) {
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double num = x2 * a0 + y2 * a1 + a2;
    const double den = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1, sd = sqrt(den);
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) {
        const double* M = D[k];
        const double d0 = M[0] * x1 + M[1] * y1 + M[2], d1 = M[3] * x1 + M[4] * y1 + M[5], d2 = M[6] * x1 + M[7] * y1 + M[8];
        const double e0 = M[0] * x2 + M[3] * y2 + M[6], e1 = M[1] * x2 + M[4] * y2 + M[7];
        const double dnum = x2 * d0 + y2 * d1 + d2;
        const double hd = a0 * d0 + a1 * d1 + b0 * e0 + b1 * e1;
        J[k] = f * (dnum - num * hd / den) / sd;
    }
    return f * num / sd;
}

// partial `lane` of the cost
MSFM_FHD double lane_cost(const double E[9], double f, const double* x1, const double* y1, const double* x2, const double* y2, const int* idx,
                          int n, int lane) {
    double c = 0.0;
    for (int j = lane; j < n; j += kLanes) {
        const int i = idx ? idx[j] : j;
        const double r = residual(E, f, x1[i], y1[i], x2[i], y2[i]);
        c = c + r * r;
    }
    return c;
}

// partial `lane` of the 21 sums
MSFM_FHD void lane_sums(const double E[9], const double D[5][9], double f, const double* x1, const double* y1, const double* x2,
                        const double* y2, const int* idx, int n, int lane, double acc[kSums]) {
MSFM_UNROLL
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int j = lane; j < n; j += kLanes) {
        const int i = idx ? idx[j] : j;
        double J[5];
        const double r = jacobian(E, D, f, x1[i], y1[i], x2[i], y2[i], J);
        int at = 0;
MSFM_UNROLL
        for (int p = 0; p < 5; ++p)
MSFM_UNROLL
            for (int q = p; q < 5; ++q) {
                acc[at] = acc[at] + J[p] * J[q];
                ++at;
            }
MSFM_UNROLL
        for (int p = 0; p < 5; ++p) acc[15 + p] = acc[15 + p] + J[p] * r;
        acc[kCostSum] = acc[kCostSum] + r * r;
    }
}

// (H + lambda diag H) x = -g from the 21 sums by a 5 x 5 Cholesky.  False: a pivot is not > 0 or x is not finite.
MSFM_FHD bool solve5(const double acc[kSums], double lambda, double x[5]) {
    double L[5][5];
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 5; ++r)
MSFM_UNROLL
        for (int c = r; c < 5; ++c) {
            L[c][r] = c == r ? acc[at] + lambda * acc[at] : acc[at];   // lower triangle
            ++at;
        }
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) {
        double dd = L[k][k];
MSFM_UNROLL
        for (int m = 0; m < k; ++m) dd = dd - L[k][m] * L[k][m];
        if (!(dd > 0.0)) return false;
        dd = sqrt(dd);
        L[k][k] = dd;
MSFM_UNROLL
        for (int r = k + 1; r < 5; ++r) {
            double s = L[r][k];
MSFM_UNROLL
            for (int m = 0; m < k; ++m) s = s - L[r][m] * L[k][m];
            L[r][k] = s / dd;
        }
    }
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) {   // L y = -g
        double s = -acc[15 + k];
MSFM_UNROLL
        for (int m = 0; m < k; ++m) s = s - L[k][m] * x[m];
        x[k] = s / L[k][k];
    }
MSFM_UNROLL
    for (int k = 4; k >= 0; --k) {   // L^T x = y
        double s = x[k];
MSFM_UNROLL
        for (int m = k + 1; m < 5; ++m) s = s - L[m][k] * x[m];
        x[k] = s / L[k][k];
    }
    bool ok = true;
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) ok = ok && msfm_pose::finite(x[k]);
    return ok;
}

// delta = (a, b) applied to s.  False: the new state is not finite.
MSFM_FHD bool apply_step(const State& s, const double x[5], State* sn) {
    const double x6[6] = {x[0], x[1], x[2], 0.0, 0.0, 0.0}, zero[3] = {0.0, 0.0, 0.0};
    double unused[3];
    bool ok = msfm_reg::cayley_update(x6, s.R, zero, sn->R, unused);
    double B[6];
    tangent_basis(s.t, B);
    const double u0 = s.t[0] + (B[0] * x[3] + B[3] * x[4]), u1 = s.t[1] + (B[1] * x[3] + B[4] * x[4]), u2 = s.t[2] + (B[2] * x[3] + B[5] * x[4]);
    const double nn = sqrt(u0 * u0 + u1 * u1 + u2 * u2);
    sn->t[0] = u0 / nn;
    sn->t[1] = u1 / nn;
    sn->t[2] = u2 / nn;
    return ok && msfm_pose::finite(sn->t[0]) && msfm_pose::finite(sn->t[1]) && msfm_pose::finite(sn->t[2]);
}

// what the statistics of a pose are reduced to (tv_pose_kernel's steps 5 and 6)
struct Stats {
    int32_t n_positive_depth, n_triangulated;
    double sum_residual, sum_angle, lo, hi;
};

// one pair: the 5 x 5 problem of msfm_ref::lm_minimise over the reduced passes of `ev`
template <class E>
struct PairProblem {
    typedef msfm_tvr::State State;
    typedef msfm_tvr::System System;
    const E& ev;
    MSFM_FHD double cost(const State& s, bool* depth) const {
        *depth = true;
        return ev.cost(s);
    }
    MSFM_FHD void linearise(const State& s, System* sys) const { ev.sums(s, sys->acc); }
    MSFM_FHD bool step(const System& sys, double lambda, const State& s, State* sn, double* d2) const {
        double x[5];
        if (!solve5(sys.acc, lambda, x) || !apply_step(s, x, sn)) return false;
        *d2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4];
        return true;
    }
    MSFM_FHD double stop_scale(const State&) const { return 1.0; }
};

MSFM_FHD void clear_refinement(msfm_two_view_refinement* r) {
    r->status = 0;
    r->stop = msfm_ref::STOP_NONE;
    r->steps = r->accepted = 0;
    r->n_positive_depth_before = r->n_triangulated_before = 0;
    r->cost_before = r->cost_after = 0.0;
}

// One pair.  `ev` owns the pair's kept list and gives the REDUCED passes, the same bits wherever it runs:
//   ev.cost(s) -> c;   ev.sums(s, acc) -> the 21 sums;   ev.stats(P, &st) -> the statistics under P = R[9] | t[3].
// old: the pair's record; *rec_out: the refined record, filled iff the result is true (it stands); *out: always filled.
template <class E>
MSFM_FHD bool refine_pair(const E& ev, const msfm_two_view_refine_params& prm, const msfm_two_view_params& tp,
                          const msfm_two_view_record& old, msfm_two_view_record* rec_out, msfm_two_view_refinement* out) {
    clear_refinement(out);
    if (!old.valid || old.n_kept < prm.min_matches) return false;
    const PairProblem<E> pb{ev};
    State s;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) s.R[k] = old.R[k];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) s.t[k] = old.t[k];
    msfm_ref::LmRun run;
    msfm_ref::lm_minimise(pb, prm.max_iters, prm.step_tol, &s, &run);
    out->status = MSFM_TVR_ELIGIBLE | (run.accepted > 0 ? MSFM_TVR_STEP_ACCEPTED : 0);
    out->stop = run.stop;
    out->steps = run.steps;
    out->accepted = run.accepted;
    out->n_positive_depth_before = old.n_positive_depth;
    out->n_triangulated_before = old.n_triangulated;
    out->cost_before = msfm_pose::canonical(run.cost_before);   // (THE NaN RULE: a cost that is NaN is never accepted, but it is handed out)
    out->cost_after = out->cost_before;
    if (run.accepted == 0) return false;
    double P[12];
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) P[k] = s.R[k];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) P[9 + k] = s.t[k];
    Stats st;
    ev.stats(P, &st);
    if (st.n_positive_depth < old.n_positive_depth || st.n_triangulated < old.n_triangulated) return false;
    msfm_pose::finish_record<1>(P, old.n_kept, st.n_positive_depth, st.n_triangulated, st.sum_residual, st.sum_angle, st.lo, st.hi, tp, rec_out);
    out->status |= MSFM_TVR_REFINED;
    out->cost_after = run.cost;
    return true;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: the reduced passes over one pair's kept matches (x1, y1, x2, y2: n entries in list order) -------------------------
struct HostEval {
    const double *x1, *y1, *x2, *y2;
    int n;
    double f, tri_max_error;
    static void tree(double* v) {
        for (int s = kLanes / 2; s >= 1; s /= 2)
            for (int l = 0; l < s; ++l) v[l] = v[l] + v[l + s];
    }
    double cost(const State& s) const {
        double E[9], v[kLanes];
        cross_mat(s.t, s.R, E);
        for (int l = 0; l < kLanes; ++l) v[l] = lane_cost(E, f, x1, y1, x2, y2, nullptr, n, l);
        tree(v);
        return v[0];
    }
    void sums(const State& s, double acc[kSums]) const {
        double E[9], D[5][9];
        linear_model(s, E, D);
        std::vector<double> part((size_t)kLanes * kSums);
        for (int l = 0; l < kLanes; ++l) lane_sums(E, D, f, x1, y1, x2, y2, nullptr, n, l, part.data() + (size_t)l * kSums);
        for (int k = 0; k < kSums; ++k) {
            double v[kLanes];
            for (int l = 0; l < kLanes; ++l) v[l] = part[(size_t)l * kSums + k];
            tree(v);
            acc[k] = v[0];
        }
    }
    void stats(const double P[12], Stats* st) const {
        const msfm_pose::HostStatistics h = msfm_pose::host_statistics(P, x1, y1, x2, y2, n, f, tri_max_error);   // (the one host copy)
        *st = Stats{h.n_positive_depth, h.n_triangulated, h.sum_residual, h.sum_angle, h.lo, h.hi};
    }
};

// (kept normalised coordinates, record, params) -> (record', refinement): *rec is rewritten iff the refined record stands
inline void refine_record(const double* x1, const double* y1, const double* x2, const double* y2, int n, double f,
                          const msfm_two_view_params& tp, const msfm_two_view_refine_params& prm, msfm_two_view_record* rec,
                          msfm_two_view_refinement* out) {
    const HostEval ev{x1, y1, x2, y2, n, f, tp.tri_max_error};
    msfm_two_view_record r;
    if (refine_pair(ev, prm, tp, *rec, &r, out)) *rec = r;
}
#endif

}  // namespace msfm_tvr
