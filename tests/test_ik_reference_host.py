"""tests/ik_reference.py checked on the host: the 50-digit kinematics against the oracle and the golden files, and the input
classes against the conditions that tests/test_gpu_ik_batch.py relies on.  No GPU.

Measured here (slot_insertion, 3 arms; run with -s for the tables):

mp_fk / mp_jac vs orc_fk / orc_jac, max |difference| per class over the three arms:
  limits 4e-16 / 1e-15, zeros 5e-324 / 7e-16, wraps 9e-16 / 1e-15, large (|q| <= 1e3 rad) 6e-14 / 7e-14;  golden rows (every 16th) 2e-15.

Exit iterations of the oracle's GradIK (orc_gradik_last_it) on hold(), 24 problems in 6 groups of four per manipulator:
  left   17 50 21 50 | 50 15 50 28 | 18 36 50 50 | 50 50 18 29 | 21 50 50 34 | 50 18 24 50      spread per group 33 35 32 32 29 32
  right  10 50 20 50 | 50 11 50 24 | 12 50 50 50 | 50 50 29 50 | 50 15 50 50 | 50 50 50 19      spread per group 40 39 38 21 35 31
  Laddering orc_gradik_max_it does NOT measure this.  It shows the last iteration at which the best iterate improved
  (gradik_last_improvement): for the same problems
  left   17 21 21 16 | 24  0 14 14 | 18  0 32 22 | 47 23 18 29 | 21 22 44 34 | 14  0 24 37
  right   0 21  0 10 | 10  0 16 24 |  0 45 43 30 | 39 13  0 34 | 32  0 10 40 | 38 47 17  0
  -- spread over 0 .. 47 for rows that run all 50 iterations as well.  By the oracle's own count, of the 512 hold problems that the 256
  golden rows of an arm give (target FK(q), and FK(q + u) with |u| <= 1e-5), 20 (left) and 10 (right) leave the loop before iteration 50,
  every one at the pose threshold; hold() is made of those that do so at the same iteration when q moves by an ulp, and of rows that run
  all 50.  In every one of about 100 early exits found (these, and targets FK(q + u) with |u| up to 3e-2) the iterate after the exit costs
  more than the best so far.

oracle_sensitivity (8 one-ulp perturbations of q), median / max per class, problems above the 1e-7 cut:
  DiffIK, 10 iterations   limits_ik  left 1e-13 / 2e-11 (0/18), right 3e-13 / 1e-9 (0/18), middle 2e-13 / 2e-10 (0/21)
                          far        left 2e-13 / 4e-12 (0/16), right 8e-15 / 6e-10 (0/16), middle 8e-14 / 4e-12 (0/16)
                          quats      left 1e-14 / 9e-14 (0/36), right 2e-14 / 4e-12 (0/36), middle 9e-15 / 3e-11 (0/36)
                          (limits_ik under seed 0 puts 1 of the right arm's 18 above the cut, 5.6 %: reselected, LIMITS_SEED = 1)
  GradIK, K = 1 / 4 / 8   hold       left max 4e-16 / 5e-13 / 2e-12, right max 4e-16 / 6e-13 / 8e-12
                          far        left max 1e-12 / 6e-12 / 4e-11, right max 2e-12 / 6e-12 / 4e-11
                          quats      left max 6e-13 / 3e-12 / 2e-11, right max 8e-13 / 3e-12 / 3e-11        (none above the cut)
  GradIK, 50 iterations   hold median 1e-8 / 9e-6 (left / right) max 1e-2, far median 3e-4 .. 5e-3 max 4e-2, quats median 2e-3 .. 6e-3
                          max 2e-2: 40 % of hold and three quarters and more of far and quats above the cut -- final GradIK joints
                          cannot be compared tightly.

Quaternion variants on the oracle (DiffIK, every arm): -q and q give bit-identical answers, the zero quaternion and (1, 0, 0, 0) give
bit-identical answers; 3 q and 1e-3 q agree with q only to the float32 rounding of the normalisation (quat2mat casts the quaternion to
float32 before it divides by the norm): answers up to 6.8e-6 apart, exactly equal in 4 of 36 comparisons."""
import os

import numpy as np
import pytest

import ik_reference as R

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def m():
    return R.orc_model()


def test_the_closed_form_exponential_is_the_matrix_exponential():
    """_exp_screw (Rodrigues, unit axis) against mp.expm of the 4 x 4 twist matrix: the reference's formula is no input of mp_fk."""
    from mpmath import mp, mpf
    for arm, joint, th in ((0, 1, 0.7), (1, 3, -2.9), (2, 6, 3.0)):
        w, v = R._screws(arm, R.model())[joint]
        Rm, p = R._exp_screw(w, v, mpf(th))
        S = mp.matrix([[0, -w[2], w[1], v[0]], [w[2], 0, -w[0], v[1]], [-w[1], w[0], 0, v[2]], [0, 0, 0, 0]]) * mpf(th)
        E = mp.expm(S)
        err = max(abs(E[i, j] - (Rm[i][j] if j < 3 else p[i])) for i in range(3) for j in range(4))
        assert err < mpf(10) ** -40, (arm, joint, err)


@pytest.mark.parametrize("arm", [0, 1, 2])
def test_mp_kinematics_agree_with_the_oracle_on_every_class(m, arm):
    classes = dict(R.fk_classes(arm))
    for name, f in (("hold", R.hold), ("far", R.far), ("quats", R.quats), ("limits_ik", R.limits_ik)):
        classes[name] = f(arm)["q"][::6]          # (rows of the golden box: a sample)
    for name, qs in classes.items():
        eT = max(np.abs(R.mp_fk(arm, q) - R.orc_fk(m, arm, q)).max() for q in qs)
        eJ = max(np.abs(R.mp_jac(arm, q) - R.orc_jac(m, arm, q)).max() for q in qs)
        print(f"{R.ARMS[arm]} {name}: {len(qs)} configurations, mp vs oracle fk {eT:.1e} jac {eJ:.1e}")
        assert eT < 1e-12 and eJ < 1e-12, (name, eT, eJ)


@pytest.mark.parametrize("arm", [0, 1, 2])
def test_mp_kinematics_agree_with_the_golden_files(arm):
    d = np.load(os.path.join(G, f"fk_jac_{R.ARMS[arm]}.npz"))
    rows = range(0, len(d["q"]), 16)
    eT = max(np.abs(R.mp_fk(arm, d["q"][i]) - d["fk"][i]).max() for i in rows)
    eJ = max(np.abs(R.mp_jac(arm, d["q"][i]) - d["jac"][i]).max() for i in rows)
    print(f"{R.ARMS[arm]}: {len(rows)} golden rows, fk {eT:.1e} jac {eJ:.1e}")
    assert eT < 1e-12 and eJ < 1e-12, (eT, eJ)


def test_classes_are_what_they_say():
    for arm in range(3):
        lo, hi = R.ranges(arm)
        q = R.limits(arm)
        assert q.shape == (3 * R.NJ[arm], R.NJ[arm]) and (q >= lo).all() and (q <= hi).all()
        for j in range(R.NJ[arm]):
            assert q[3 * j, j] == lo[j] and q[3 * j + 1, j] == hi[j] and q[3 * j + 2, j] == 0.5 * (lo[j] + hi[j])
        z = R.zeros(arm)
        assert not np.signbit(z[0]).any() and np.signbit(z[1]).all() and (z[:2] == 0).all() and (z[2] == 1e-310).all()
        assert np.abs(R.wraps(arm)).min() >= np.pi and np.abs(R.wraps(arm)).max() == 2 * np.pi + 1e-9
        assert np.abs(R.large(arm)).max() == 1e3 and np.abs(R.large(arm)).min() >= 10.0
        assert sum(len(v) for v in R.fk_classes(arm).values()) in (45, 48)
        p = R.far(arm)
        for i in range(len(p["q"])):
            T = R.mp_fk(arm, p["q"][i])
            assert abs(np.linalg.norm(p["pos"][i] - T[:3, 3]) - 2.0) < 1e-12
        p = R.quats(arm)
        assert (p["quat"][p["variant"] == 4] == 0).all() and np.array_equal(p["quat"][1::6], -p["quat"][0::6])
        b = R.mixed_batch(arm)
        assert b["q"].shape == (257, R.NJ[arm]) and b["pos"].shape == (257, 3) and b["quat"].shape == (257, 4)


def test_two_arm_blob_keeps_the_camera_arm():
    """avsim_api.hip fill_ik takes the camera arm's null-space posture q0 from qpos_home[ik_qadr[2]] = qpos_home[16 .. 22].  A 2-arm model
    hides the camera arm (its base is moved away, compile.py) but keeps its joints: nq, ik_qadr and qpos_home are the 3-arm model's, so
    these entries are the arm's posture and not object coordinates, and avsim_ik(arm = 2) is as meaningful on a 2-arm handle as
    avsim_fk_jac(arm = 2).  Only the arm's screw axes and site pose differ (the moved base)."""
    m3, m2 = R.model("slot_insertion", 3), R.model("slot_insertion", 2)
    assert int(m2["num_arms"][0]) == 2 and int(m2["nq"][0]) == int(m3["nq"][0]) == 37
    adr = np.asarray(m2["ik_qadr"]).reshape(3, 7)
    assert np.array_equal(adr, np.asarray(m3["ik_qadr"]).reshape(3, 7)) and adr[2].tolist() == list(range(16, 23))
    assert np.array_equal(m2["qpos_home"], m3["qpos_home"])
    assert np.array_equal(np.asarray(m2["qpos_home"])[16:23], [0.0, -0.8, 0.8, 0.0, 0.5, 0.0, 0.0])
    assert set(int(a) for a in np.asarray(m2["objects_qposadr"]).reshape(-1)).isdisjoint(range(16, 23))
    assert np.array_equal(m2["ik_range"], m3["ik_range"]) and np.array_equal(m2["ik_w0"][:2], m3["ik_w0"][:2])
    assert not np.array_equal(m2["ik_p0"][2], m3["ik_p0"][2])


@pytest.mark.parametrize("arm", [0, 1])
def test_hold_mixes_the_exits_of_every_group_of_four(m, arm):
    """The exit iteration is orc_gradik_last_it, the oracle's own count.  Laddering orc_gradik_max_it (gradik_last_improvement) does not give
    it: on these problems it shows values spread over 10 .. 50 for the rows that never leave the loop as well -- the best iterate of a
    secant descent stops improving long before the loop ends.  By the oracle's count only 4 % of the hold problems leave early."""
    p = R.hold(arm)
    n = len(p["q"])
    ex = [R.gradik_exit(m, arm, p["q"][i], p["pos"][i], p["quat"][i]) for i in range(n)]
    ladder = [R.gradik_last_improvement(m, arm, p["q"][i], p["pos"][i], p["quat"][i]) for i in range(n)]
    spread = [max(ex[i:i + 4]) - min(ex[i:i + 4]) for i in range(0, n, 4)]
    print(R.ARMS[arm], "exit iterations", ex, "spread per group of four", spread, "last improvement by laddering", ladder)
    assert n == 24 and min(spread) >= 5, (ex, spread)
    assert ex == R.HOLD_EXITS[arm]
    assert all(l <= e for l, e in zip(ladder, ex))
    early = [e for e in ex if e < 50]
    assert len(early) >= 8 and len(set(early)) >= 6          # (rows that do leave, at iterations of their own)
    # GradIK does move the joints when asked to hold the pose: this is no trivial path
    moved = max(np.abs(R.orc_gradik(m, arm, p["q"][i], p["pos"][i], p["quat"][i]) - p["q"][i]).max() for i in range(n))
    assert moved > 1e-3, moved


def _row(s):
    return "median %.1e max %.1e, above the cut %d/%d" % (np.median(s), s.max(), (s > R.SENS_CUT).sum(), len(s))


def test_sensitivity_table_and_the_cut(m):
    """The table of the module docstring; the cut is a condition on the INPUTS: at most 5 % of a class may lie above 1e-7 at the iteration
    counts at which tests/test_gpu_ik_batch.py compares with the oracle (DiffIK 10, GradIK 8).  A class that breaks it is reselected."""
    for arm in range(3):
        for name, f in (("limits_ik", R.limits_ik), ("far", R.far), ("quats", R.quats)):
            s = R.sensitivities(m, arm, 0, 10, f(arm))
            print(f"DiffIK 10 {R.ARMS[arm]} {name}: {_row(s)}")
            assert (s > R.SENS_CUT).mean() <= 0.05, (arm, name, s)
    for arm in range(2):
        for name, f in (("hold", R.hold), ("far", R.far), ("quats", R.quats)):
            for K in (1, 4, 8, 50):
                s = R.sensitivities(m, arm, 1, K, f(arm))
                print(f"GradIK {K} {R.ARMS[arm]} {name}: {_row(s)}")
                if K <= 8:
                    assert (s > R.SENS_CUT).mean() <= 0.05, (arm, name, K, s)


@pytest.mark.parametrize("arm", [0, 1, 2])
def test_quaternion_variants_on_the_oracle(m, arm):
    """What tests/test_gpu_ik_batch.py may ask of the device: -q and q exactly alike, zero and identity exactly alike, 3 q and 1e-3 q alike
    only to float32 rounding.  Bound of the latter: the float32 cast of a scaled quaternion rounds differently (6e-8 relative per entry), the
    target matrix moves by a few float32 ulps, <= 5e-7; the damped least-squares step turns an orientation error e into at most
    k_ori e / (2 sqrt(damping)) = 45 e of joint motion per iteration, ten iterations: 2.3e-4."""
    p = R.quats(arm)
    worst, exact = 0.0, 0
    for b in range(len(p["q"]) // 6):
        o = [R.orc_diffik(m, arm, p["q"][6 * b + v], p["pos"][6 * b + v], p["quat"][6 * b + v]) for v in range(6)]
        assert np.array_equal(o[0], o[1]) and np.array_equal(o[4], o[5])
        assert not np.array_equal(o[0], o[5])          # (the target is not the identity: the zero quaternion is a different problem)
        for v in (2, 3):
            e = np.abs(o[v] - o[0]).max()
            worst, exact = max(worst, e), exact + (e == 0)
            assert e < 2.3e-4, (b, v, e)
    print(f"{R.ARMS[arm]}: scaled quaternions move the oracle's DiffIK answer by up to {worst:.1e}; exactly equal in {exact} of 12")
    assert worst > 0          # float32 rounding of the normalisation, not exact: stated in test_gpu_ik_batch.py
