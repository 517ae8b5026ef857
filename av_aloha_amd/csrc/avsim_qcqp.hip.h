// avsim_qcqp.hip.h -- the friction block of an elliptic contact in the noslip pass (mj_solNoSlip [EXT]): the exact minimiser of
// 1/2 x'Ax + x'b over the cone section sum (x_j / mu_j)^2 <= fn^2 (mju_QCQP2 / mju_QCQP), fn = the normal force held fixed.
// The arithmetic of ONE block on ONE lane: no cross-lane operation, no LDS, no global pointer -- pgs_groups, qcqp_slide_octet and the
// per-tree pass (avsim_phys.hip.h) gather a block their own way and call in here, and tests/hostshim compiles this file for the CPU
// (tests/test_qcqp_host.py).  `mode` is the option "qcqp_tridiag": 0 = MuJoCo's evaluation, 1 = the tridiagonal form with MuJoCo's
// Newton steps on the multiplier, 2 = the tridiagonal form with the secular step.
#pragma once
#include "avsim_math.hip.h"

namespace avs {

// convergence thresholds of the multiplier iteration in the noslip QCQP: MuJoCo's absolute 1e-10 in double; in float a relative
// part on top, since v.v - r^2 and the multiplier carry 1e-7 relative rounding
// t / d with 1 / d at hand.  The product kernel (float) multiplies: a division there is ten instructions (range scaling around
// v_rcp_f32), and the multiplier iteration of the noslip QCQP is thirty divisions per step.  The parity kernel (double) divides, as
// the oracle does.
template <typename T> AVS_DEV T qdiv(T t, T d, T dinv) { return sizeof(T) == 4 ? t * dinv : t / d; }
#if defined(__HIPCC__)
AVS_DEV float qrsqrt(float x) { return __builtin_amdgcn_rsqf(x); }
#else
AVS_DEV float qrsqrt(float x) { return 1.0f / sqrt(x); }      // (a host build of this header)
#endif
AVS_DEV double qrsqrt(double x) { return 1.0 / sqrt(x); }
template <typename T> struct QTol;
template <> struct QTol<double> { static constexpr double abs = 1e-10, rel = 0.0; };
template <> struct QTol<float> { static constexpr float abs = 1e-10f, rel = 2e-6f; };

// Step of the multiplier iteration of a sliding contact's QCQP, |y(la)| = r with y = -(A + la I)^-1 b.  MuJoCo's mju_QCQP takes
// Newton steps on |y|^2 - r^2 from la = 0 (val / (2 y.w), w = (A + la I)^-1 y); that function is strongly convex in la and the
// iteration needs about nine steps on a dragging arm.  1 / |y(la)| is nearly linear in la (the trust-region secular equation, More
// and Sorensen 1983), so Newton on 1 / r - 1 / |y| reaches the SAME root in two to four steps, also monotonically from the left:
// delta = (|y| - r) / r * |y|^2 / (y.w), with |y| - r taken as val / (|y| + r).  Product mode (f32, option qcqp_tridiag = 2); the
// f64 parity kernel keeps MuJoCo's steps.
template <typename T> AVS_DEV T secular_step(T val, T r2, T r, T yw) {
    const T yy = val + r2, ny = sqrt(yy);
    return val * yy / ((ny + r) * r * yw);
}

// A block's data from the lanes that own its rows (row j + 1 of the contact = friction row j): bc(x, l) is lane l's x -- a wave-wide
// broadcast in pgs_groups, an octet's in qcqp_slide_octet.  res = this lane's row residual, f0 its force, muinv 1 / mu, inv 1 / A_rr,
// acs its couplings to the rows before it (word 0 = to the normal row).  -> A (n x n in 5 x 5, identity padded), b = res - A f,
// d = mu, the forces and the residuals.
template <typename real, typename BC>
AVS_DEV void qcqp_gather(BC bc, int n, real res, real f0, real muinv, real inv, const real* acs, real (&Aq)[5][5], real (&bq)[5], real (&dq)[5],
                         real (&oldf)[5], real (&resq)[5]) {
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const bool in = j < n;
        resq[j] = in ? bc(res, j + 1) : real(0);
        oldf[j] = in ? bc(f0, j + 1) : real(0);
        const real mi = bc(muinv, j + 1);
        dq[j] = in ? real(1) / mi : real(1);
        const real di = bc(inv, j + 1);
        Aq[j][j] = in ? real(1) / di : real(1);
#pragma unroll
        for (int k = 0; k < j; k++) { const real c = in ? bc(acs[k + 1], j + 1) : real(0); Aq[j][k] = c; Aq[k][j] = c; }
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        real t = resq[j];
#pragma unroll
        for (int k = 0; k < 5; k++) t -= (j < n && k < n) ? Aq[j][k] * oldf[k] : real(0);
        bq[j] = t;
    }
}

// an active constraint's solution exactly onto the ellipsoid sum (v_j / d_j)^2 = r2
template <typename real>
AVS_DEV void qcqp_onto_ellipsoid(real (&v)[5], const real (&dq)[5], int n, real r2) {
    real sq = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) sq += j < n ? v[j] * v[j] / (dq[j] * dq[j]) : real(0);
    const real sc = sqrt(r2 / tmax(real(1e-15), sq));
#pragma unroll
    for (int j = 0; j < 5; j++) v[j] *= sc;
}

// mju_QCQP2 [EXT]: two friction rows.  The problem is scaled so that the constraint becomes |y| <= fn, then the iteration on the
// multiplier la of the constraint with the inverse of the two-by-two block written out.  -> v, exactly on the ellipsoid when the
// constraint is active (la != 0; the return value); v = 0 when the block is singular (determinant below 1e-10).
template <typename real>
AVS_DEV bool qcqp2(real A00, real A10, real A11, real b0, real b1, real dq0, real dq1, real fn, int mode, real& v0, real& v1) {
    const real r2 = fn * fn, vtol = QTol<real>::abs + QTol<real>::rel * r2;
    real la = 0;
    const real b1s = b0 * dq0, b2s = b1 * dq1;
    const real A11s = A00 * dq0 * dq0, A22s = A11 * dq1 * dq1, A12s = A10 * dq0 * dq1;
    real y1 = 0, y2 = 0;
    bool singular = false;
    for (int iter = 0; iter < 20; iter++) {
        const real det = (A11s + la) * (A22s + la) - A12s * A12s;
        if (det < real(1e-10)) { singular = true; break; }
        const real detinv = real(1) / det, P11 = (A22s + la) * detinv, P22 = (A11s + la) * detinv, P12 = -A12s * detinv;
        y1 = -P11 * b1s - P12 * b2s;
        y2 = -P12 * b1s - P22 * b2s;
        const real val = y1 * y1 + y2 * y2 - r2;
        if (val < vtol) break;
        const real yw = P11 * y1 * y1 + 2 * P12 * y1 * y2 + P22 * y2 * y2;
        const real delta = mode == 2 ? secular_step(val, r2, fn, yw) : val / (2 * yw);
        if (delta < QTol<real>::abs + QTol<real>::rel * la) break;
        la += delta;
    }
    v0 = singular ? real(0) : y1 * dq0;
    v1 = singular ? real(0) : y2 * dq1;
    const bool active = !singular && la != 0;
    if (active) {
        real v[5] = {v0, v1, 0, 0, 0};
        const real d[5] = {dq0, dq1, 1, 1, 1};
        qcqp_onto_ellipsoid(v, d, 2, r2);
        v0 = v[0]; v1 = v[1];
    }
    return active;
}

// mju_QCQP [EXT], three to five friction rows, modes 1 and 2.  mju_QCQP's Newton iteration on the multiplier needs
// y = -(As + la I)^-1 bs and (As + la I)^-1 y for a dozen values of la.  MuJoCo factors As + la I afresh every time (a 5 x 5
// Cholesky: a chain of ~150 dependent instructions, 1.2 k cycles, redundantly on every lane).  Here As is reduced once to
// tridiagonal form by three Householder reflections, As = H T H^T; (As + la I)^-1 = H (T + la I)^-1 H^T, |y| and y . w are the same
// in the rotated basis, and T + la I is factored by the four-step LDL^T recurrence: the same iterates up to rounding, a quarter of
// the instructions per iterate.  Singularity is MuJoCo's pivot rule at la = 0 (`singular`: the flag make_constraints left with the
// block's inverse; the pivots only grow with la).  -> y (scaled: the force is y_j d_j; 0 when singular), la, nit += the iterates.
template <typename real>
AVS_DEV void qcqp5_tridiag(const real (&Aq)[5][5], const real (&bq)[5], const real (&dq)[5], int n, real fn, int mode, bool singular, real (&y)[5],
                           real& la, int& nit) {
    const real r2 = fn * fn, vtol = QTol<real>::abs + QTol<real>::rel * r2;
    real As[5][5], cs[5], w[5], hv[3][5], hb[3];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        cs[j] = j < n ? bq[j] * dq[j] : real(0);
        y[j] = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) As[j][k] = (j < n && k < n) ? Aq[j][k] * dq[j] * dq[k] : (j == k ? real(1) : real(0));
    }
    if (singular) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        real sigma = 0;
#pragma unroll
        for (int i = k + 2; i < 5; i++) sigma += As[i][k] * As[i][k];
        const real x0 = As[k + 1][k];
#pragma unroll
        for (int i = 0; i < 5; i++) hv[k][i] = 0;
        hb[k] = 0;
        if (sigma != real(0)) {       // (wave-uniform: the column is tridiagonal already otherwise)
            const real nrm = sqrt(x0 * x0 + sigma), alpha = x0 > 0 ? -nrm : nrm;
            hv[k][k + 1] = x0 - alpha;
#pragma unroll
            for (int i = k + 2; i < 5; i++) hv[k][i] = As[i][k];
            const real beta = real(2) / (hv[k][k + 1] * hv[k][k + 1] + sigma);
            hb[k] = beta;
            real pv[5], vp = 0;
#pragma unroll
            for (int i = k + 1; i < 5; i++) {
                real t = 0;
#pragma unroll
                for (int j = k + 1; j < 5; j++) t += As[i][j] * hv[k][j];
                pv[i] = beta * t;
                vp += hv[k][i] * pv[i];
            }
            const real K = real(0.5) * beta * vp;
#pragma unroll
            for (int i = k + 1; i < 5; i++) pv[i] -= K * hv[k][i];
#pragma unroll
            for (int i = k + 1; i < 5; i++)
#pragma unroll
                for (int j = k + 1; j <= i; j++) { As[i][j] -= hv[k][i] * pv[j] + pv[i] * hv[k][j]; As[j][i] = As[i][j]; }
            As[k + 1][k] = alpha; As[k][k + 1] = alpha;
#pragma unroll
            for (int i = k + 2; i < 5; i++) { As[i][k] = 0; As[k][i] = 0; }
            // right-hand side into the rotated basis
            real t = 0;
#pragma unroll
            for (int i = k + 1; i < 5; i++) t += hv[k][i] * cs[i];
            t *= beta;
#pragma unroll
            for (int i = k + 1; i < 5; i++) cs[i] -= t * hv[k][i];
        }
    }
    const real b0 = As[1][0], b1 = As[2][1], b2 = As[3][2], b3 = As[4][3];
    for (int iter = 0; iter < 20; iter++) {
        nit++;
        // LDL^T of T + la I (la on the contact's own dimensions only, as in mju_QCQP's padded loops)
        const real d0 = As[0][0] + la, r0 = real(1) / d0, l0 = b0 * r0;
        const real d1 = As[1][1] + la - l0 * b0, r1 = real(1) / d1, l1 = b1 * r1;
        const real d2 = As[2][2] + la - l1 * b1, r2_ = real(1) / d2, l2 = b2 * r2_;
        const real d3 = As[3][3] + (3 < n ? la : real(0)) - l2 * b2, r3 = real(1) / d3, l3 = b3 * r3;
        const real d4 = As[4][4] + (4 < n ? la : real(0)) - l3 * b3, r4 = real(1) / d4;
        real z0 = -cs[0], z1 = -cs[1] - l0 * z0, z2 = -cs[2] - l1 * z1, z3 = -cs[3] - l2 * z2, z4 = -cs[4] - l3 * z3;
        y[4] = z4 * r4; y[3] = z3 * r3 - l3 * y[4]; y[2] = z2 * r2_ - l2 * y[3]; y[1] = z1 * r1 - l1 * y[2]; y[0] = z0 * r0 - l0 * y[1];
        real val = -r2;
#pragma unroll
        for (int i = 0; i < 5; i++) val += y[i] * y[i];
        if (val < vtol) break;
        z0 = y[0]; z1 = y[1] - l0 * z0; z2 = y[2] - l1 * z1; z3 = y[3] - l2 * z2; z4 = y[4] - l3 * z3;
        w[4] = z4 * r4; w[3] = z3 * r3 - l3 * w[4]; w[2] = z2 * r2_ - l2 * w[3]; w[1] = z1 * r1 - l1 * w[2]; w[0] = z0 * r0 - l0 * w[1];
        real yw = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) yw += y[i] * w[i];
        const real delta = mode == 2 ? secular_step(val, r2, fn, yw) : val / (2 * yw);
        if (delta < QTol<real>::abs + QTol<real>::rel * la) break;
        la += delta;
    }
    // back to the contact's basis: y <- H y
#pragma unroll
    for (int k = 2; k >= 0; k--) {
        real t = 0;
#pragma unroll
        for (int i = k + 1; i < 5; i++) t += hv[k][i] * y[i];
        t *= hb[k];
#pragma unroll
        for (int i = k + 1; i < 5; i++) y[i] -= t * hv[k][i];
    }
}

// mju_QCQP [EXT], mode 0: MuJoCo's own evaluation, a Cholesky factorisation of As + la I per iterate (the f64 parity mode's default:
// the oracle's arithmetic, operation for operation).  -> y, la and nit as above; returns true when a pivot fell below 1e-10 (singular).
template <typename real>
AVS_DEV bool qcqp5_cholesky(const real (&Aq)[5][5], const real (&bq)[5], const real (&dq)[5], int n, real fn, real (&y)[5], real& la, int& nit) {
    const real r2 = fn * fn, vtol = QTol<real>::abs + QTol<real>::rel * r2;
    bool singular = false;
    real As[5][5], bs[5], L[5][5], w[5], rd[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        bs[j] = j < n ? bq[j] * dq[j] : real(0);
        y[j] = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) As[j][k] = (j < n && k < n) ? Aq[j][k] * dq[j] * dq[k] : (j == k ? real(1) : real(0));
    }
    for (int iter = 0; iter < 20; iter++) {
        nit++;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            real dd = As[j][j] + (j < n ? la : real(0));
#pragma unroll
            for (int k = 0; k < j; k++) dd -= L[j][k] * L[j][k];
            if (j < n && dd < real(1e-10)) singular = true;
            dd = tmax(dd, real(1e-30));
            if (sizeof(real) == 4) { rd[j] = qrsqrt(dd); dd = dd * rd[j]; }
            else { dd = sqrt(dd); rd[j] = real(1) / dd; }
            L[j][j] = dd;
#pragma unroll
            for (int i = j + 1; i < 5; i++) {
                real t = As[i][j];
#pragma unroll
                for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
                L[i][j] = qdiv(t, dd, rd[j]);
            }
        }
        if (singular) break;
#pragma unroll
        for (int i = 0; i < 5; i++) { real t = -bs[i]; for (int k = 0; k < i; k++) t -= L[i][k] * y[k]; y[i] = qdiv(t, L[i][i], rd[i]); }
#pragma unroll
        for (int i = 4; i >= 0; i--) { real t = y[i]; for (int k = i + 1; k < 5; k++) t -= L[k][i] * y[k]; y[i] = qdiv(t, L[i][i], rd[i]); }
        real val = -r2;
#pragma unroll
        for (int i = 0; i < 5; i++) val += y[i] * y[i];
        if (val < vtol) break;
#pragma unroll
        for (int i = 0; i < 5; i++) { real t = y[i]; for (int k = 0; k < i; k++) t -= L[i][k] * w[k]; w[i] = qdiv(t, L[i][i], rd[i]); }
#pragma unroll
        for (int i = 4; i >= 0; i--) { real t = w[i]; for (int k = i + 1; k < 5; k++) t -= L[k][i] * w[k]; w[i] = qdiv(t, L[i][i], rd[i]); }
        real deriv = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) deriv += y[i] * w[i];
        deriv *= -2;
        const real delta = -val / deriv;
        if (delta < QTol<real>::abs + QTol<real>::rel * la) break;
        la += delta;
    }
    return singular;
}

// change of the cost when the forces go from oldf to v [EXT: costChange]; an update that would raise it by more than 1e-10 is not made
template <typename real>
AVS_DEV real qcqp_cost_change(const real (&Aq)[5][5], const real (&v)[5], const real (&oldf)[5], const real (&resq)[5], int n) {
    real change = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        real t = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) t += (j < n && k < n) ? Aq[j][k] * (v[k] - oldf[k]) : real(0);
        change += j < n ? (v[j] - oldf[j]) * (real(0.5) * t + resq[j]) : real(0);
    }
    return change;
}

}  // namespace avs
