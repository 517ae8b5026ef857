// The device's noslip QCQP arithmetic (av_aloha_amd/csrc/avsim_qcqp.hip.h) compiled for the host with the oracle's floating-point
// rules (-ffp-contract=off), behind a C entry point per precision.  Test infrastructure: tests/test_qcqp_host.py compares the modes
// with each other and with the oracle's orc_qcqp (oracle/orc.h) on random blocks.
#include "../../av_aloha_amd/csrc/avsim_qcqp.hip.h"

using namespace avs;

// One friction block the way pgs_groups solves it once the block is gathered: no friction force without a normal force, two rows
// through qcqp2 (two != 0) or padded to five like the larger blocks, mode = the option qcqp_tridiag, the solution of an active
// constraint put onto the ellipsoid.  A: n x n row-major, b, mu: n.  -> v[5], the active flag, the iterates taken.
template <typename T>
static void block(int n, const double* A, const double* b, const double* mu, double fn_, int mode, int two, double* v_out, int* active_out, int* nit_out) {
    T Aq[5][5], bq[5], dq[5], v[5] = {0, 0, 0, 0, 0};
    for (int j = 0; j < 5; j++) {
        bq[j] = j < n ? (T)b[j] : T(0);
        dq[j] = j < n ? (T)mu[j] : T(1);
        for (int k = 0; k < 5; k++) Aq[j][k] = (j < n && k < n) ? (T)A[n * j + k] : (j == k ? T(1) : T(0));
    }
    const T fn = (T)fn_;
    int nit = 0;
    bool active = false;
    if (!(fn < T(1e-15))) {
        if (two) active = qcqp2<T>(Aq[0][0], Aq[1][0], Aq[1][1], bq[0], bq[1], dq[0], dq[1], fn, mode, v[0], v[1]);
        else {
            T y[5], la = 0;
            bool singular = false;
            if (mode) {
                // the flag make_constraints leaves with the block's inverse: MuJoCo's pivot rule on the scaled block at multiplier 0
                T L[5][5];
                for (int j = 0; j < n; j++) {
                    T dd = Aq[j][j] * dq[j] * dq[j];
                    for (int k = 0; k < j; k++) dd -= L[j][k] * L[j][k];
                    if (dd < T(1e-10)) { singular = true; break; }
                    dd = sqrt(dd);
                    L[j][j] = dd;
                    for (int i = j + 1; i < n; i++) {
                        T t = Aq[i][j] * dq[i] * dq[j];
                        for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
                        L[i][j] = t / dd;
                    }
                }
                qcqp5_tridiag(Aq, bq, dq, n, fn, mode, singular, y, la, nit);
            } else singular = qcqp5_cholesky(Aq, bq, dq, n, fn, y, la, nit);
            for (int j = 0; j < 5; j++) v[j] = (singular || !(j < n)) ? T(0) : y[j] * dq[j];
            active = !singular && la != 0;
            if (active) qcqp_onto_ellipsoid(v, dq, n, fn * fn);
        }
    }
    for (int j = 0; j < 5; j++) v_out[j] = (double)v[j];
    *active_out = active;
    *nit_out = nit;
}

template <typename T>
static void blocks(int count, int n, const double* A, const double* b, const double* mu, const double* fn, int mode, int two, double* v, int* active, int* nit) {
    for (int c = 0; c < count; c++) block<T>(n, A + (size_t)c * n * n, b + (size_t)c * n, mu + (size_t)c * n, fn[c], mode, two, v + 5 * (size_t)c, active + c, nit + c);
}

extern "C" void dev_qcqp_f64(int count, int n, const double* A, const double* b, const double* mu, const double* fn, int mode, int two, double* v, int* active, int* nit) {
    blocks<double>(count, n, A, b, mu, fn, mode, two, v, active, nit);
}
extern "C" void dev_qcqp_f32(int count, int n, const double* A, const double* b, const double* mu, const double* fn, int mode, int two, double* v, int* active, int* nit) {
    blocks<float>(count, n, A, b, mu, fn, mode, two, v, active, nit);
}
