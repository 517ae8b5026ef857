"""The noslip pass's QCQP arithmetic (av_aloha_amd/csrc/avsim_qcqp.hip.h: qcqp2, qcqp5_cholesky, qcqp5_tridiag, the projection onto the
ellipsoid) compiled for the HOST by g++ with the oracle's floating-point rules (tests/hostshim/host_qcqp.cpp) and run on random friction
blocks against the oracle's orc_qcqp (mju_QCQP2 / mju_QCQP of oracle/orc_dyn.c) and against itself across the three modes of the option
qcqp_tridiag -- no GPU needed.

Inputs, per n in {2, 3, 4, 5}: 2400 blocks, seed fixed.  The friction coefficients are the rows of pair_friction of the compiled models
(models/*.avm: sliding 0.6 .. 2, torsional 0.005 .. 0.05, rolling 1e-4 .. 1e-2), fn is log-uniform in 1e-3 .. 1e2 N (a resting peg .. a
gripper's squeeze).  The SCALED block D A D is drawn with eigenvalues log-uniform in 0.05 .. 50 and A = D^-1 (D A D) D^-1, because
MuJoCo's singularity rule (a Cholesky pivot of the scaled block below 1e-10) would otherwise call every block with a rolling coefficient
singular.  b puts the unconstrained minimiser at |y| / fn in 0.05 .. 0.9 ("inside", 45 %) or in 1.1 .. 30 ("sliding", 35 %); 15 % of the
blocks are L L' with L lower triangular, small dyadic entries, powers of two on the diagonal and 0 as its last entry, their coefficients
rounded down to powers of two ("singular": every step of the factorisation is exact in float and in double, the last pivot is 0), and
5 % have fn below 1e-15 (0, 1e-16, 1e-300), where the call sites skip the solve."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from orc_ffi import ROOT, dp, ip, lib
from test_oracle_physics import read_blob

COUNT = 2400
NS = (2, 3, 4, 5)
# 10 x the largest relative difference (max_j |v_j - ref_j| / max_j |ref_j|) from mode 0, the oracle's arithmetic, measured on these inputs
# in f64.  Mode 1 (the same Newton steps on the tridiagonal form): 7.14e-13 (n = 3).  Mode 2 (the secular step): 3.74e-5 (n = 4) -- the
# iteration ends on the ABSOLUTE test |y|^2 - r^2 < 1e-10, which at fn = 1e-3 is 1e-4 of r^2, and the two kinds of step end at different
# points below it; the projection onto the ellipsoid then keeps the difference in direction.  qcqp2 against qcqp5_cholesky on n = 2
# measured 7.31e-14 (modes 0 and 1) and 8.83e-6 (mode 2): under the same bounds.
MODE_BOUND = {0: 7.2e-12, 1: 7.2e-12, 2: 3.8e-4}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostshim") / "libhostqcqp.so")
    shim = os.path.join(ROOT, "tests", "hostshim")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + shim,
                           "-o", so, os.path.join(shim, "host_qcqp.cpp")])
    return C.CDLL(so)


def model_frictions():
    rows = []
    for path in sorted(glob.glob(os.path.join(ROOT, "models", "*.avm"))):
        rows.append(read_blob(path)["pair_friction"].reshape(-1, 5))
    return np.unique(np.concatenate(rows), axis=0)


@pytest.fixture(scope="module")
def cases():
    """n -> dict(A [COUNT, n, n], b, mu [COUNT, n], fn [COUNT], cls [COUNT]: 0 inside, 1 sliding, 2 singular, 3 no normal force)"""
    rng = np.random.default_rng(20)
    fric = model_frictions()
    assert fric.min() > 0
    out = {}
    for n in NS:
        mu = fric[rng.integers(len(fric), size=COUNT)][:, :n].copy()
        cls = rng.choice(4, size=COUNT, p=[0.45, 0.35, 0.15, 0.05])
        fn = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), COUNT))
        fn[cls == 3] = rng.choice([0.0, 1e-16, 1e-300], size=int((cls == 3).sum()))
        A, b = np.zeros((COUNT, n, n)), np.zeros((COUNT, n))
        for c in range(COUNT):
            if cls[c] == 2:
                Lf = np.tril(rng.integers(-8, 9, size=(n, n)) / 8.0, -1) + np.diag(rng.choice([0.5, 1.0, 2.0], size=n))
                Lf[n - 1, n - 1] = 0.0
                As = Lf @ Lf.T
                mu[c] = 2.0 ** np.floor(np.log2(mu[c]))
            else:
                Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
                As = (Q * np.exp(rng.uniform(np.log(0.05), np.log(50.0), n))) @ Q.T
            As = 0.5 * (As + As.T)
            rho = rng.uniform(0.05, 0.9) if cls[c] == 0 else np.exp(rng.uniform(np.log(1.1), np.log(30.0)))
            y0 = rng.normal(size=n)
            y0 *= rho * max(fn[c], 1e-3) / np.linalg.norm(y0)
            A[c] = As / np.outer(mu[c], mu[c])
            b[c] = -(As @ y0) / mu[c]
        out[n] = dict(A=A, b=b, mu=mu, fn=fn, cls=cls)
    return out


def run_host(host, real, case, n, mode, two=0):
    f = getattr(host, "dev_qcqp_" + real)
    v, act, nit = np.zeros((COUNT, 5)), np.zeros(COUNT, dtype=np.int32), np.zeros(COUNT, dtype=np.int32)
    f(COUNT, n, dp(case["A"]), dp(case["b"]), dp(case["mu"]), dp(case["fn"]), mode, two, dp(v), ip(act), ip(nit))
    assert not v[:, n:].any()
    return v[:, :n], act.astype(bool)


@pytest.fixture(scope="module")
def oracle(cases):
    """n -> (v, active) of orc_qcqp followed by orc_noslip's own steps around it: nothing without a normal force, an active constraint's
    solution onto the ellipsoid (the same expressions in numpy, IEEE double)"""
    L = lib()
    L.orc_qcqp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int]
    out = {}
    for n, case in cases.items():
        v, act = np.zeros((COUNT, n)), np.zeros(COUNT, dtype=bool)
        for c in range(COUNT):
            if case["fn"][c] < 1e-15:
                continue
            act[c] = L.orc_qcqp(v[c].ctypes.data, case["A"][c].ctypes.data, case["b"][c].ctypes.data, case["mu"][c].ctypes.data, case["fn"][c], n)
        s = np.zeros(COUNT)
        for j in range(n):
            s = s + v[:, j] * v[:, j] / (case["mu"][:, j] * case["mu"][:, j])
        s = np.sqrt(case["fn"] * case["fn"] / np.maximum(1e-15, s))
        v[act] *= s[act, None]
        out[n] = (v, act)
    return out


def rel_diff(v, ref):
    return np.abs(v - ref).max(axis=1) / np.maximum(np.abs(ref).max(axis=1), 1e-300)


def test_every_class_of_block_is_there(cases, oracle):
    """inside, sliding and singular by what the oracle makes of the blocks, at least 10 % each"""
    for n in NS:
        v, act = oracle[n]
        has_fn = cases[n]["fn"] >= 1e-15
        sliding = act
        inside = has_fn & ~act & v.any(axis=1)
        singular = has_fn & ~act & ~v.any(axis=1)
        print(n, "inside %.3f sliding %.3f singular %.3f no normal force %.3f" % (inside.mean(), sliding.mean(), singular.mean(), (~has_fn).mean()))
        assert inside.mean() >= 0.1 and sliding.mean() >= 0.1 and singular.mean() >= 0.1
        assert np.array_equal(inside, cases[n]["cls"] == 0) and np.array_equal(sliding, cases[n]["cls"] == 1) and np.array_equal(singular, cases[n]["cls"] == 2)


def test_f64_mode_0_is_the_oracles_arithmetic(host, cases, oracle):
    """qcqp2 (n = 2) and qcqp5_cholesky (n = 3, 4, 5) in double give orc_qcqp's result and active flag bit for bit"""
    for n in NS:
        v, act = run_host(host, "f64", cases[n], n, 0, two=int(n == 2))
        ref, ract = oracle[n]
        assert np.array_equal(act, ract)
        assert np.array_equal(v, ref), (n, rel_diff(v, ref).max())


def test_f64_modes_1_and_2_reach_the_root_of_mode_0(host, cases):
    for n in NS:
        ref, ract = run_host(host, "f64", cases[n], n, 0, two=int(n == 2))
        for mode in (1, 2):
            v, act = run_host(host, "f64", cases[n], n, mode, two=int(n == 2))
            assert np.array_equal(act, ract), (n, mode)
            d = rel_diff(v, ref).max()
            print("n %d mode %d: %.3g" % (n, mode, d))
            assert d <= MODE_BOUND[mode], (n, mode, d)


def test_qcqp2_equals_the_padded_cholesky_evaluation(host, cases):
    for mode in (0, 1, 2):
        v2, act2 = run_host(host, "f64", cases[2], 2, mode, two=1)
        v5, act5 = run_host(host, "f64", cases[2], 2, 0, two=0)
        assert np.array_equal(act2, act5), mode
        d = rel_diff(v2, v5).max()
        print("mode %d: %.3g" % (mode, d))
        assert d <= MODE_BOUND[mode], (mode, d)


@pytest.mark.parametrize("real", ["f64", "f32"])
def test_active_results_lie_on_the_ellipsoid_and_inactive_ones_inside(host, cases, real):
    """active: |sum (v_j / mu_j)^2 - fn^2| <= 8 ulp of fn^2 in the result's precision (the sum evaluated in extended precision from the
    coefficients the routine saw); inactive: the kernel's own test val < QTol::abs + QTol::rel r^2"""
    T = np.float64 if real == "f64" else np.float32
    tol_abs, tol_rel = (1e-10, 0.0) if real == "f64" else (np.float32(1e-10), np.float32(2e-6))
    for n in NS:
        mu = cases[n]["mu"].astype(T).astype(np.longdouble)
        r2 = (cases[n]["fn"].astype(T) * cases[n]["fn"].astype(T)).astype(np.longdouble)
        for mode in (0, 1, 2):
            for two in ((0, 1) if n == 2 else (0,)):
                v, act = run_host(host, real, cases[n], n, mode, two)
                val = ((v.astype(np.longdouble) / mu) ** 2).sum(axis=1) - r2
                ulp = np.spacing(r2.astype(T)).astype(np.longdouble)
                print("%s n %d mode %d two %d: active %d, off the ellipsoid by at most %.2f ulp" % (real, n, mode, two, act.sum(), (np.abs(val[act]) / ulp[act]).max()))
                assert act.sum() >= 0.1 * COUNT
                assert (np.abs(val[act]) <= 8 * ulp[act]).all(), (n, mode, two)
                assert (val[~act] < tol_abs + tol_rel * r2[~act]).all(), (n, mode, two)
