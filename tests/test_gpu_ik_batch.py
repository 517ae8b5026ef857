"""The IK kernels off their golden shapes (k_fk_jac, k_ik, k_gradik_ctrl, k_cart_ctrl; avsim_ik.hip.h): ragged batches, rows of one
wave that leave GradIK's loop at different iterations, joint values at the limits, at 0, at +-pi and far beyond, degenerate
quaternions, and the control kernels' own addressing.  Inputs and the 50-digit kinematics: tests/ik_reference.py (checked on the
host by tests/test_ik_reference_host.py, which also holds the sensitivity table and the exit iterations of hold()).

Most of what is asked is an exact equality: a problem's answer does not depend on where in a batch it stands, with whom it shares a
wave, or which kernel computes it.  Where the device is compared with the oracle the bound is per problem,
max(1e-11, 1e3 x oracle_sensitivity): the probe moves q by one ulp once, the device differs from the oracle by a rounding in every
sincos and every contraction, about a hundred operations per iteration."""
import numpy as np
import pytest

import ik_reference as R
from avsim_test_util import blob
from gpu_util import device_handle, torch as T

pytestmark = pytest.mark.gpu

GUARD = 8
PREFIXES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 67)


class Side:
    """One handle, fed numpy arrays (host I/O) or torch tensors on its device (AVSIM_IO_DEVICE, as tests/test_gpu_io_modes.py).  In device
    mode an output tensor has GUARD rows behind row n, filled with a NaN pattern that must come back untouched; the input tensors hold
    exactly n rows."""

    def __init__(self, device_mode, num_arms=3):
        from av_aloha_amd import _ffi
        self.ffi, self.device_mode = _ffi, device_mode
        if device_mode:
            self.T = T
            self.h, self.dev = device_handle("slot_insertion", 8, num_arms=num_arms)
        else:
            self.h = _ffi.Handle(blob("slot_insertion", num_arms), 8)
        self.L = self.h.L

    def _in(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return self.T.from_numpy(a.copy()).to(self.dev) if self.device_mode else a

    def _out(self, n, w):
        if not self.device_mode:
            return np.full((n, w), np.nan)
        pat = (np.uint64(0x7FF8DEAD00000000) + np.arange((n + GUARD) * w, dtype=np.uint64)).view(np.float64).reshape(n + GUARD, w)
        return self.T.from_numpy(pat.copy()).to(self.dev), pat

    def _back(self, o, n):
        if not self.device_mode:
            return o
        t, pat = o
        self.T.cuda.current_stream().synchronize()
        got = t.cpu().numpy()
        assert np.array_equal(got[n:].view(np.uint64), pat[n:].view(np.uint64)), "rows behind row n were written"
        return got[:n].copy()

    @staticmethod
    def _p(o):
        return o[0] if isinstance(o, tuple) else o

    def fk_jac(self, arm, q, want_T=True, want_J=True):
        n, nj = q.shape
        qi = self._in(q)
        T = self._out(n, 16) if want_T else None
        J = self._out(n, 6 * nj) if want_J else None
        self.h.check(self.L.avsim_fk_jac(self.h.h, arm, n, self.ffi.ptr(qi), self.ffi.ptr(self._p(T)) if want_T else None,
                                         self.ffi.ptr(self._p(J)) if want_J else None))
        return (self._back(T, n) if want_T else None), (self._back(J, n) if want_J else None)

    def ik(self, arm, controller, iters, p):
        n, nj = p["q"].shape
        qi, pi, xi = self._in(p["q"]), self._in(p["pos"]), self._in(p["quat"])
        o = self._out(n, nj)
        self.h.check(self.L.avsim_ik(self.h.h, arm, controller, iters, n, self.ffi.ptr(qi), self.ffi.ptr(pi), self.ffi.ptr(xi),
                                     self.ffi.ptr(self._p(o))))
        return self._back(o, n)

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def sides():
    s = {"host": Side(False), "device": Side(True)}
    yield s
    for x in s.values():
        x.close()


@pytest.fixture(scope="module")
def orc():
    return R.orc_model()


def fk_inputs(arm):
    c = R.fk_classes(arm)
    return np.ascontiguousarray(np.concatenate([c["limits"], c["zeros"], c["wraps"], c["large"]]))


# ---- 1. FK and the Jacobian against the 50-digit reference ---------------------------------------------------------------------
@pytest.mark.parametrize("arm", [0, 1, 2])
def test_fk_jac_against_the_50_digit_reference(sides, arm):
    """limits, zeros (0, -0.0, 1e-310), wraps (+-pi, +-(2 pi + 1e-9)) and large (|q| <= 1e3 rad): 45 configurations of a manipulator, 48
    of the camera arm.  atol 1e-12, the golden test's bound: at most 7 joints x a few dozen roundings x 1.1e-16 x entries <= 2 m is about
    3e-14 (at |q| = 1e3 the translation term th v rounds at 1e-13 per joint: measured on the oracle 6e-14)."""
    q = fk_inputs(arm)
    n, nj = q.shape
    assert n in (45, 48)
    Tref = np.array([R.mp_fk(arm, x) for x in q])
    Jref = np.array([R.mp_jac(arm, x) for x in q])
    for name, s in sides.items():
        T, J = s.fk_jac(arm, q)
        eT, eJ = np.abs(T.reshape(n, 4, 4) - Tref).max(), np.abs(J.reshape(n, 6, nj) - Jref).max()
        print(f"{R.ARMS[arm]} {name}: device vs 50-digit fk {eT:.1e} jac {eJ:.1e}")
        np.testing.assert_allclose(T.reshape(n, 4, 4), Tref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(J.reshape(n, 6, nj), Jref, rtol=0, atol=1e-12)
        assert np.array_equal(T[:, 12:16], np.tile([0.0, 0.0, 0.0, 1.0], (n, 1)))
        # either output works without the other
        T1, none = s.fk_jac(arm, q, want_J=False)
        none2, J1 = s.fk_jac(arm, q, want_T=False)
        assert none is None and none2 is None and np.array_equal(T1, T) and np.array_equal(J1, J)


# ---- 2. batch position does not matter, bit for bit ----------------------------------------------------------------------------
CONFIGS = ([("fk", a, 0) for a in range(3)] + [("diffik", a, 0) for a in range(3)]
           + [("gradik", a, k) for a in range(2) for k in (0, 4)])


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}-{R.ARMS[c[1]]}-{c[2]}")
def test_batch_position_does_not_matter(sides, mode, cfg):
    """257 problems (hold, far, quats, golden rows; for FK the q classes in front) solved at once, then as prefixes of every size round
    the wave (64), the GradIK block (4 problems) and the 16-lane row, as a random permutation, and every 16th problem alone: each
    problem's output is the same bits.  This runs the tail code: `ii = live ? i : n - 1`, the idle rows that shadow the last problem,
    the store guard and the (n + 3) / 4 grid."""
    kind, arm, iters = cfg
    s = sides[mode]
    batch = R.mixed_batch(arm)
    if kind == "fk":
        qall = np.ascontiguousarray(np.concatenate([fk_inputs(arm), batch["q"]])[:257])

        def solve(idx):
            T, J = s.fk_jac(arm, np.ascontiguousarray(qall[idx]))
            return np.concatenate([T, J], axis=1)
    else:
        def solve(idx):
            return s.ik(arm, 0 if kind == "diffik" else 1, iters, R.take(batch, idx))
    big = solve(np.arange(257))
    assert np.isfinite(big).all()
    for n in PREFIXES:
        assert np.array_equal(solve(np.arange(n)), big[:n]), f"prefix n = {n}"
    perm = np.random.default_rng(3).permutation(257)
    assert np.array_equal(solve(perm), big[perm]), "permutation"
    for i in range(0, 257, 16):
        assert np.array_equal(solve(np.array([i])), big[i:i + 1]), f"problem {i} alone"


# ---- 3. mixed exits inside a wave ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", [0, 1])
def test_gradik_rows_of_a_wave_that_finish_at_different_iterations(sides, arm):
    """The hold() groups of four at the default 50 iterations: one group is one wave, and in each the oracle leaves the loop at iteration
    10 .. 36 for one or two rows and never for the others (ik_reference.HOLD_EXITS, held by tests/test_ik_reference_host.py; such exits
    are rare, 4 % of the hold targets, so the rows are picked).  A row that has finished keeps evaluating behind `if (!done)` while the
    others go on.  Each problem's answer in its mixed group equals its answer in a wave of four copies of itself (all rows leave
    together) and its answer alone (three idle rows shadow it), exactly.  (Implied by the batch-position test; kept apart so that a
    failure names the `done` logic.)

    What this notices, tried once each on a scratch build: a finished row that is not frozen (`if (!done)` made unconditional) fails
    here for both arms -- problems 2 (left) and 0 (right) move by 3e-4 and 3e-3, as the oracle without its breaks predicts for 2 of the
    12 and 3 of the 8 early rows.  Moving only the update of `best` out of `if (!done)` changes no answer, here or anywhere found: a
    frozen row re-evaluates the one iterate that follows its exit, and that iterate never cost less than the best so far (see
    tests/test_ik_reference_host.py), so no output shows that mutation."""
    s = sides["host"]
    p = R.hold(arm)
    for g in range(0, len(p["q"]), 4):
        mixed = s.ik(arm, 1, 0, R.take(p, np.arange(g, g + 4)))
        for k in range(4):
            same = s.ik(arm, 1, 0, R.take(p, np.full(4, g + k)))
            alone = s.ik(arm, 1, 0, R.take(p, np.array([g + k])))
            assert np.array_equal(same, np.tile(alone, (4, 1))), (g, k)
            assert np.array_equal(mixed[k], alone[0]), f"problem {g + k}: mixed group {mixed[k]} vs alone {alone[0]}"


# ---- 4. against the oracle on the new classes ----------------------------------------------------------------------------------
def _against_oracle(s, orc, arm, controller, iters, name, p):
    """Device vs oracle on one class: per-problem bound, the cut, the ranges.  Returns (worst err / bound, worst err / sensitivity)."""
    dev = s.ik(arm, controller, iters, p)
    fn = R.orc_diffik if controller == 0 else R.orc_gradik
    k = iters if iters else (10 if controller == 0 else 50)
    ref = np.array([fn(orc, arm, p["q"][i], p["pos"][i], p["quat"][i], k) for i in range(len(dev))])
    sens = R.sensitivities(orc, arm, controller, k, p)
    keep = sens <= R.SENS_CUT
    assert (~keep).mean() <= 0.05, (name, sens)
    err = np.abs(dev - ref).max(axis=1)
    bound = np.maximum(1e-11, 1e3 * sens)
    governed = keep & (1e3 * sens > 1e-11)
    ratio = (err[governed] / sens[governed]).max() if governed.any() else 0.0
    print(f"{R.ARMS[arm]} {'DiffIK' if controller == 0 else 'GradIK'} {k} {name}: max err {err[keep].max():.1e}, worst err / bound "
          f"{(err / bound)[keep].max():.2g}, worst err / sensitivity where the sensitivity sets the bound {ratio:.2g} ({governed.sum()} problems)")
    lo, hi = R.ranges(arm)
    assert (dev >= lo).all() and (dev <= hi).all(), name
    assert (err[keep] <= bound[keep]).all(), (name, np.argmax(err / bound), err, bound)
    return dev


def _quat_identities(dev, p):
    """quats(): problem 6 b + v is target b with its quaternion as it is, negated, x 3, x 1e-3, all zero, (1, 0, 0, 0)."""
    v = [dev[k::6] for k in range(6)]
    assert np.array_equal(v[0], v[1]), "q and -q"
    assert np.array_equal(v[4], v[5]), "the zero quaternion and the identity"          # (quat2mat_xyzw's branch n < 8.88e-16)
    assert not np.array_equal(v[0], v[5])
    # 3 q and 1e-3 q: alike only to the float32 rounding of the normalisation -- so the oracle (test_quaternion_variants_on_the_oracle,
    # which derives the bound 2.3e-4 for DiffIK; GradIK's first iterations move less), so the device
    for k in (2, 3):
        assert np.abs(v[k] - v[0]).max() < 2.3e-4, k


@pytest.mark.parametrize("arm", [0, 1, 2])
def test_diffik_against_the_oracle_on_limits_far_and_quats(sides, orc, arm):
    """DiffIK at its 10 iterations.  Measured: worst err / sensitivity 3.0 (middle, quats), worst err / bound 0.003; per class in MEASURED
    below.  -q equals q and the zero quaternion equals (1, 0, 0, 0) bit for bit; 3 q and 1e-3 q equal q only to float32
    rounding of the normalisation (oracle and device alike: up to 6.8e-6 apart)."""
    s = sides["host"]
    for name, f in (("limits_ik", R.limits_ik), ("far", R.far), ("quats", R.quats)):
        dev = _against_oracle(s, orc, arm, 0, 0, name, f(arm))
        if name == "quats":
            _quat_identities(dev, f(arm))


@pytest.mark.parametrize("K", [1, 4, 8])
@pytest.mark.parametrize("arm", [0, 1])
def test_gradik_against_the_oracle_on_hold_far_and_quats(sides, orc, arm, K):
    """GradIK stopped after K = 1, 4, 8 iterations, the oracle through orc_gradik_max_it = K.  Measured: worst err / sensitivity 3.7 (left,
    far, K = 1), worst err / bound 0.0037; per class in MEASURED below.

    What this notices, tried once each on a scratch build: difference points that lose the sign of one side (gs = +step on every lane)
    fail all six cases, K = 1 included (errors of 0.1 rad).  Flipping the sign of gs on both sides changes no bit and cannot be noticed:
    the gradient, the two secant points and the secant ratio change sign together, x = local - (-g) (-jd)."""
    s = sides["host"]
    for name, f in (("hold", R.hold), ("far", R.far), ("quats", R.quats)):
        dev = _against_oracle(s, orc, arm, 1, K, name, f(arm))
        if name == "quats":
            _quat_identities(dev, f(arm))


# ---- 5. the control kernels are the IK entry points plus addressing ------------------------------------------------------------
def _cart_case(N, seed):
    """qpos [N, nq] with every arm joint uniform inside its range, and a 23-D action per env whose targets differ per env and per arm:
    hold-like (the arm's pose moved by <= 1 mm / 1e-3 rad) or far-like (2 m, 3 rad), alternating over env + arm; triggers random."""
    md = R.model()
    rng = np.random.default_rng(seed)
    qadr = np.asarray(md["ik_qadr"]).reshape(3, 7)
    qpos = np.tile(np.asarray(md["qpos_home"], dtype=np.float64), (N, 1))
    act = np.zeros((N, 23))
    for arm in range(3):
        lo, hi = R.ranges(arm)
        q = rng.uniform(lo, hi, size=(N, R.NJ[arm]))
        qpos[:, qadr[arm, :R.NJ[arm]]] = q
        off = (0, 8, 16)[arm]
        for i in range(N):
            p, Rm = R._pose(arm, q[i].astype(np.float32).astype(np.float64))
            if (i + arm) % 2:
                p, Rm = p + 2.0 * R._unit(rng), R._rotvec(3.0 * R._unit(rng)) @ Rm
            else:
                p, Rm = p + 1e-3 * R._unit(rng), R._rotvec(1e-3 * R._unit(rng)) @ Rm
            act[i, off:off + 3], act[i, off + 3:off + 7] = p, R._wxyz(Rm)
        if arm < 2:
            act[:, off + 7] = rng.uniform(0, 1, size=N)
    return qpos, act


_CART = {}
MODES = {"reference": 0, "dls": 1}          # _ffi.IK_REFERENCE, _ffi.IK_DLS


def _cart_run(N, f64):
    """step_cartesian(nsub = 0) in both modes, with the envs as drawn and permuted, and avsim_ik on the joints the handle holds
    (get_state: the handle's reals as doubles), default iteration counts, cast to the handle's real.  One run per (N, real), shared."""
    if (N, f64) in _CART:
        return _CART[N, f64]
    from av_aloha_amd.sim import BatchedSim
    md = R.model()
    real = np.float64 if f64 else np.float32
    qadr = np.asarray(md["ik_qadr"]).reshape(3, 7)
    sim = BatchedSim("slot_insertion", 3, N, f64=f64)
    rec = {"real": real, "perm": np.random.default_rng(N).permutation(N)}
    try:
        qpos, act = _cart_case(N, 100 + N)
        for mname, mode in MODES.items():
            for tag, order in (("as drawn", np.arange(N)), ("permuted", rec["perm"])):
                sim.set_state(qpos=qpos[order])
                sim.step_cartesian(act[order], mode, nsub=0)
                held, _, ctrl, _ = sim.get_state()
                assert np.array_equal(held, qpos[order].astype(real).astype(np.float64))          # (no substep: the joints stand)
                a = act[order]
                want = []
                for arm, ao in enumerate((0, 8, 16)):
                    nj = R.NJ[arm]
                    controller = 1 if (mname == "reference" and arm < 2) else 0
                    q = np.ascontiguousarray(held[:, qadr[arm, :nj]])
                    pos, quat = np.ascontiguousarray(a[:, ao:ao + 3]), np.ascontiguousarray(a[:, ao + 3:ao + 7])
                    out = np.zeros((N, nj))
                    sim.h.check(sim.h.L.avsim_ik(sim.h.h, arm, controller, 0, N, q.ctypes.data, pos.ctypes.data, quat.ctypes.data, out.ctypes.data))
                    want.append(out.astype(real).astype(np.float64))
                rec[mname, tag] = (ctrl, want, a)
    finally:
        sim.close()
    _CART[N, f64] = rec
    return rec


CART_CASES = [pytest.param(N, f64, id=f"{N}-{'f64' if f64 else 'f32'}") for N in (1, 5, 67) for f64 in (False, True)]
CTRL_OFF = (0, 7, 14)


def _assert_arm_exact(rec, mname, arm):
    for tag in ("as drawn", "permuted"):
        ctrl, want, _ = rec[mname, tag]
        got = ctrl[:, CTRL_OFF[arm]:CTRL_OFF[arm] + R.NJ[arm]]
        d = np.abs(got - want[arm])
        assert np.array_equal(got, want[arm]), (f"{mname} mode, envs {tag}, arm {arm}: {(d.max(axis=1) > 0).sum()} of {len(d)} envs differ from "
                                                f"avsim_ik, max |ctrl - avsim_ik| = {d.max():.3e}")


@pytest.mark.parametrize("N,f64", CART_CASES)
def test_cartesian_control_addressing_grippers_and_gradik_arms(N, f64):
    """k_gradik_ctrl and the addressing of both control kernels (action offsets 0 / 8 / 16, ctrl offsets 0 / 7 / 14, qadr, the (real) cast,
    blockIdx.y + arm0) at N = 1, 5, 67 -- no multiple of 4 or 64 -- on float and double handles, with joints, targets (hold-like and
    far-like) and triggers that differ per env and per arm.  The manipulators' ctrl entries in the reference mode are EXACTLY avsim_ik's
    GradIK answers (50 iterations) cast to the real; the grippers are unnorm(1 - trigger) from the blob's grip_range within one ulp of the
    real in both modes; permuting the envs permutes ctrl in both modes.  Measured on the MI355X: exact in all six cases."""
    md = R.model()
    rec = _cart_run(N, f64)
    real = rec["real"]
    glo, ghi = [float(x) for x in np.asarray(md["grip_range"]).reshape(-1)[:2]]
    for arm in (0, 1):
        _assert_arm_exact(rec, "reference", arm)
    for mname in MODES:
        ctrl, want, a = rec[mname, "as drawn"]
        for arm, ao in ((0, 0), (1, 8)):
            g = ((1.0 - a[:, ao + 7]) * (ghi - glo) + glo).astype(real)
            assert (np.abs(ctrl[:, CTRL_OFF[arm] + 6].astype(real) - g) <= np.spacing(np.abs(g))).all(), (mname, arm)
        assert np.array_equal(rec[mname, "permuted"][0], ctrl[rec["perm"]]), mname
        # a swapped offset shows: every arm's answer is another
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], want[2][:, :6]) and not np.array_equal(want[1], want[2][:, :6])


@pytest.mark.parametrize("N,f64", CART_CASES)
def test_cartesian_control_diffik_of_the_manipulators(N, f64):
    """The manipulators' diffik<double, 6> in the DLS mode (arms 0 and 1) is EXACTLY avsim_ik's DiffIK (10 iterations) cast to the real:
    one kernel, k_cart_ctrl, serves both.  Measured on the MI355X: exact in all six cases."""
    rec = _cart_run(N, f64)
    for arm in (0, 1):
        _assert_arm_exact(rec, "dls", arm)


@pytest.mark.parametrize("N,f64", CART_CASES)
def test_cartesian_control_diffik_of_the_camera_arm(N, f64):
    """The camera arm's 7-DoF DiffIK (arm 2, both modes) is EXACTLY avsim_ik's, cast to the real.

    This test found the two apart on a double handle: while avsim_ik had a DiffIK kernel of its own, 1 of 1, 2 of 5 and 36 of 67 envs
    differed, max |ctrl - avsim_ik| 6.7e-15, 8.9e-15 and 4.5e-11 (both modes, envs permuted or not; a float handle rounds it away).
    The cause was contraction, not addressing: avsim_api.hip is compiled with multiply-adds fused as the compiler sees fit, it chose
    differently in the two kernels' inlined copies of diffik<double, 7>, and a library built with -ffp-contract=off agreed.  Since then
    k_cart_ctrl is the one DiffIK kernel behind both entry points (addressing and real type are its arguments), so the equality holds
    by construction, for the manipulators too.  avsim_ik's camera-arm DiffIK answers moved by up to 7e-12 with that (they are the
    control path's now); ctrl of float and double handles in both modes, the manipulators' DiffIK and GradIK kept their bits."""
    rec = _cart_run(N, f64)
    for mname in MODES:
        _assert_arm_exact(rec, mname, 2)


# ---- 6. a 2-arm handle ---------------------------------------------------------------------------------------------------------
def test_the_camera_arm_on_a_two_arm_handle():
    """A 2-arm blob carries all three arms' kinematic tables, and its qpos keeps the hidden camera arm's joints: qpos_home[16 .. 22] is the
    3-arm model's posture (test_two_arm_blob_keeps_the_camera_arm, host), so fill_ik's null-space posture q0 of arm 2 is meaningful and
    avsim_ik(arm = 2) answers there as on a 3-arm handle.  Pinned: FK / Jacobian of arm 2 against the 50-digit reference built from the
    2-arm blob's own tables, and DiffIK of arm 2 against the oracle on the 2-arm model under the per-problem bound."""
    md2 = R.model("slot_insertion", 2)
    s = Side(False, num_arms=2)
    try:
        q = fk_inputs(2)
        n = len(q)
        T, J = s.fk_jac(2, q)
        Tref = np.array([R.mp_fk(2, x, md2) for x in q])
        Jref = np.array([R.mp_jac(2, x, md2) for x in q[::4]])
        np.testing.assert_allclose(T.reshape(n, 4, 4), Tref, rtol=0, atol=1e-12)
        np.testing.assert_allclose(J.reshape(n, 6, 7)[::4], Jref, rtol=0, atol=1e-12)
        orc2 = R.orc_model(2)
        p = R.far(2)
        dev = s.ik(2, 0, 0, p)
        ref = np.array([R.orc_diffik(orc2, 2, p["q"][i], p["pos"][i], p["quat"][i], 10, md2) for i in range(len(dev))])
        sens = np.array([R.oracle_sensitivity(lambda x, i=i: R.orc_diffik(orc2, 2, x, p["pos"][i], p["quat"][i], 10, md2), p["q"][i], seed=i)
                         for i in range(len(dev))])
        keep = sens <= R.SENS_CUT
        err = np.abs(dev - ref).max(axis=1)
        assert (~keep).mean() <= 0.05 and (err[keep] <= np.maximum(1e-11, 1e3 * sens)[keep]).all(), (err, sens)
    finally:
        s.close()


MEASURED = """Device vs oracle on the MI355X (host-I/O handle), per class: max err; worst err / sensitivity over the problems whose bound the
sensitivity sets (1e3 x sensitivity > 1e-11; the others are held to 1e-11).  No problem of any class lies above the 1e-7 cut, and the
worst err / bound is 0.0037: the device stays within four one-ulp sensitivities of the oracle where 1e3 are allowed.

FK / Jacobian vs the 50-digit reference, max |difference|: left 2.7e-14 / 2.5e-14, right 2.3e-14 / 2.5e-14, middle 3.8e-14 / 6.0e-14 (all of
it in the `large` class; bound 1e-12), the same through the host and the device handle.

DiffIK, 10 iterations   limits_ik  left 1.4e-11; 0.71   right 8.6e-10; 1.2   middle 8.0e-11; 1.4
                        far        left 2.0e-12; 1.2    right 1.6e-10; 1.5   middle 2.0e-12; 2.1
                        quats      left 1.1e-13; 1.6    right 1.3e-12; 0.83  middle 2.6e-11; 3.0
GradIK, K = 1           hold       left 0 (the answer is q: no first iterate beats the pose already held)   right 0
                        far        left 1.6e-12; 3.7    right 4.3e-12; 1.8
                        quats      left 4.9e-13; 1.3    right 3.4e-13; 3.0
GradIK, K = 4           hold       left 2.4e-13; 0.93   right 4.9e-13; 0.87
                        far        left 3.6e-12; 2.2    right 9.2e-12; 2.5
                        quats      left 1.6e-12; 1.0    right 8.8e-13; 1.2
GradIK, K = 8           hold       left 1.6e-12; 1.2    right 2.1e-12; 1.0
                        far        left 4.0e-11; 2.7    right 3.1e-11; 1.8
                        quats      left 1.3e-11; 0.93   right 7.2e-12; 1.8

Control kernels vs avsim_ik (item 5): exact for GradIK (both manipulators), for the 6-DoF DiffIK, for the grippers (within one ulp, as
asked) and under permutation, at N = 1, 5, 67 on float and double handles; for the camera arm's 7-DoF DiffIK since one kernel serves
avsim_step_cartesian and avsim_ik (test_cartesian_control_diffik_of_the_camera_arm: 4.5e-11 apart before, contraction)."""
