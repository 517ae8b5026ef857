"""The physics kernel compiled for one model (csrc/avsim_phys_spec.hip, option "phys_specialised") against the generic kernel.

The specialised k_phys has the model's LDS layout and table offsets as compile-time constants; everything it computes is the generic
kernel's arithmetic at other addresses-as-immediates, so the two must agree to the last bit: state, observations, rewards,
diagnostics and exported contacts, after every env-step.  What can go wrong is addressing, at any batch size, so the cases are small:
two full workgroups of eight waves, a ragged last workgroup, and the small-batch path (one wave per workgroup, which moves the table
image's LDS base).  phys_specialised = 2 ("require") must refuse -- error status, message, state untouched -- every launch that would
take the generic kernel; the default (1) runs those launches generically, equal to 0."""
import numpy as np
import pytest

from av_aloha_amd import workloads as W
from test_oracle_physics import model_dict

pytestmark = pytest.mark.gpu

STEPS = 3


def _home_poses(sim, md):
    ch = np.asarray(md["ctrl_home"], dtype=np.float64)
    Ts = []
    for arm, sl in ((0, slice(0, 6)), (1, slice(7, 13)), (2, slice(14, 21))):
        q = np.ascontiguousarray(ch[sl])[None]
        T = np.empty((1, 16))
        sim.h.check(sim.h.L.avsim_fk_jac(sim.h.h, arm, 1, q.ctypes.data, T.ctypes.data, None))
        Ts.append(T)
    return W.home_poses(Ts)


def _snapshot(sim, ap, rw, su):
    out = list(sim.get_state()) + [ap, rw, su, sim.diag()]
    out += list(sim.contacts())
    return [np.array(x, copy=True) for x in out]


NAMES = ("qpos", "qvel", "ctrl", "warmstart", "agent_pos", "reward", "success", "diag", "ncon", "contact pairs", "contact dist")


def _run(task, arms, n, options, f64=False):
    """STEPS env-steps of the task's benchmark workload (ids 0..n-1); the snapshot after every step."""
    from av_aloha_amd import _ffi
    from av_aloha_amd.sim import BatchedSim
    ids = np.arange(n)
    md = model_dict(task, arms)
    sim = BatchedSim(task, arms, n, f64=f64, options=dict({"solver": 1, "export_contacts": 1}, **options))
    seed = {"slot_insertion": 1000, "hook_package": 3000}.get(task, 5000)
    sim.reset(W.object_poses(task, ids, seed))
    snaps = []
    if task == "slot_insertion" and arms == 3:      # config 2: Cartesian sinusoid targets through the DLS IK
        home = _home_poses(sim, md)
        for t in range(STEPS):
            snaps.append(_snapshot(sim, *sim.step_cartesian(W.sinusoid_actions(home, ids, n, t), _ffi.IK_DLS)))
    else:                                           # config 4: joint-space random walk
        acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], ids, STEPS, sim.nj, seed)
        for t in range(STEPS):
            snaps.append(_snapshot(sim, *sim.step(acts[t])))
    sim.close()
    return snaps


def _assert_identical(a, b, what):
    assert len(a) == len(b) == STEPS
    for t, (sa, sb) in enumerate(zip(a, b)):
        for name, x, y in zip(NAMES, sa, sb):
            assert x.shape == y.shape and np.array_equal(x, y), f"{what}: {name} differs after env-step {t} ({np.sum(x != y)} entries)"
    assert np.isfinite(a[-1][0]).all()


# N = 16: two full workgroups of eight waves; N = 13: a ragged last workgroup; N = 5 without the option: one wave per workgroup
SHAPES = [(16, {"waves_per_block": 8}), (13, {"waves_per_block": 8}), (5, {})]


@pytest.mark.parametrize("task,arms", [("slot_insertion", 3), ("hook_package", 2)])
@pytest.mark.parametrize("n,opts", SHAPES, ids=["n16_wpb8", "n13_wpb8", "n5_small_batch"])
def test_specialised_kernel_bit_identical_to_generic(task, arms, n, opts):
    generic = _run(task, arms, n, dict(opts, phys_specialised=0))
    spec = _run(task, arms, n, dict(opts, phys_specialised=2))
    _assert_identical(generic, spec, f"{task}_{arms}arms N={n}")
    # (not a trivial agreement: the envs moved, and differently from each other)
    assert np.abs(generic[-1][1]).max() > 0 and not np.array_equal(generic[-1][0][0], generic[-1][0][1])


REFUSED = {
    "model without a spec": ("insert_peg", 2, {}, False),
    "layout changed by option": ("slot_insertion", 3, {"maxefc": 96}, False),
    "f64 handle": ("slot_insertion", 3, {}, True),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_require_mode_refuses_generic_launch_and_default_runs_it(case):
    from av_aloha_amd import _ffi
    from av_aloha_amd.sim import BatchedSim
    task, arms, opts, f64 = REFUSED[case]
    n = 4
    ids = np.arange(n)
    md = model_dict(task, arms)
    sim = BatchedSim(task, arms, n, f64=f64, options={"solver": 1})
    for k, v in opts.items():
        sim.set_option(k, v)
    sim.reset(W.object_poses(task, ids, 5000))
    acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], ids, 1, sim.nj, 5000)
    before = [x.copy() for x in sim.get_state()] + [sim.get_latch()]
    sim.set_option("phys_specialised", 2)
    with pytest.raises(_ffi.AvsimError) as ei:
        sim.step(acts[0])
    assert "phys_specialised" in str(ei.value) and "generic" in str(ei.value), str(ei.value)
    after = list(sim.get_state()) + [sim.get_latch()]
    for x, y in zip(before, after):
        assert np.array_equal(x, y), f"{case}: the refused step changed the state"
    sim.close()
    # default (1): the same handle set-up runs, on the generic kernel -- equal to phys_specialised = 0 to the last bit
    _assert_identical(_run(task, arms, n, dict(opts, phys_specialised=0), f64=f64), _run(task, arms, n, dict(opts), f64=f64), case)


@pytest.mark.parametrize("case", ["layout changed by option", "f64 handle"])
def test_require_mode_refuses_before_ik_reset_or_set_state_touch_the_state(case):
    """The Cartesian step's IK writes ctrl, reset and set_state write the whole state, all ahead of the physics launch: a refused call
    must not have run them."""
    from av_aloha_amd import _ffi
    from av_aloha_amd.sim import BatchedSim
    task, arms, opts, f64 = REFUSED[case]
    n = 4
    ids = np.arange(n)
    md = model_dict(task, arms)
    sim = BatchedSim(task, arms, n, f64=f64, options={"solver": 1})
    for k, v in opts.items():
        sim.set_option(k, v)
    poses = W.object_poses(task, ids, 1000)
    sim.reset(poses)
    home = _home_poses(sim, md)
    sim.step_cartesian(W.sinusoid_actions(home, ids, n, 0), _ffi.IK_DLS)      # away from the reset state, ctrl set by the IK
    before = [x.copy() for x in sim.get_state()] + [sim.get_latch(), sim.get_reset_poses()]
    sim.set_option("phys_specialised", 2)
    moved = [x + 0.01 for x in before[:4]]
    calls = {
        "step_cartesian": lambda: sim.step_cartesian(W.sinusoid_actions(home, ids, n, 40), _ffi.IK_DLS),
        "step_cartesian (reference IK)": lambda: sim.step_cartesian(W.sinusoid_actions(home, ids, n, 40), _ffi.IK_REFERENCE),
        "reset": lambda: sim.reset(W.object_poses(task, ids, 7000)),
        "set_state": lambda: sim.set_state(*moved),
        "set_qpos": lambda: sim.set_qpos(moved[0]),
        "step_ctrl": lambda: sim.step_ctrl(),
    }
    for name, call in calls.items():
        with pytest.raises(_ffi.AvsimError) as ei:
            call()
        assert "phys_specialised" in str(ei.value), (name, str(ei.value))
        after = list(sim.get_state()) + [sim.get_latch(), sim.get_reset_poses()]
        for what, x, y in zip(("qpos", "qvel", "ctrl", "warmstart", "latch", "reset poses"), before, after):
            assert np.array_equal(x, y), f"{case}: refused {name} changed {what}"
    sim.set_option("phys_specialised", 1)      # the same calls go through again
    sim.step_cartesian(W.sinusoid_actions(home, ids, n, 40), _ffi.IK_DLS)
    assert not np.array_equal(sim.get_state()[2], before[2])
    sim.close()


def test_default_handle_takes_the_specialised_kernel():
    from av_aloha_amd.sim import BatchedSim
    n = 4
    ids = np.arange(n)
    md = model_dict("slot_insertion", 3)
    sim = BatchedSim("slot_insertion", 3, n, options={"solver": 1})
    sim.reset(W.object_poses("slot_insertion", ids, 1000))
    acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], ids, 2, sim.nj, 1000)
    sim.step(acts[0])                       # default: phys_specialised = 1
    sim.set_option("phys_specialised", 2)   # "require" does not object: the launch takes the model's own kernel
    sim.step(acts[1])
    assert np.isfinite(sim.get_state()[0]).all()
    with pytest.raises(Exception):
        sim.set_option("phys_specialised", 3)
    sim.close()
