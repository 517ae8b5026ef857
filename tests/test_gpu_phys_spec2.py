"""Stage two of the per-model physics kernels (csrc/avsim_phys_spec.hip): dims and solver configuration as compile-time constants, the
table image at LDS offset 0.

What can go wrong is addressing and kernel selection, at any batch size, so the cases are small:

* the table base: in a per-model kernel the image sits in FRONT of the env records, whatever the workgroup's shape.  One, three and eight
  waves per workgroup with N = 1, 7 and 11 cover a lone wave, ragged last workgroups and full ones; phys_specialised = 2 must equal
  phys_specialised = 0 to the last bit on everything a step produces, after every step;
* kernel selection: a handle whose solver option is off the default the kernel was compiled for must not take it -- refused under
  phys_specialised = 2 (state untouched), run by the generic kernel under 1 (equal to 0), and taken again once the option is back;
* the launches without substeps (reset, set_state, the pose pass of the depth renderer) go through the same kernel."""
import numpy as np
import pytest

from av_aloha_amd import workloads as W
from test_gpu_phys_spec import _assert_identical, _run
from test_oracle_physics import model_dict

pytestmark = pytest.mark.gpu

MODELS = [("slot_insertion", 3), ("hook_package", 2)]


@pytest.mark.parametrize("task,arms", MODELS)
@pytest.mark.parametrize("wpb", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 7, 11])
def test_table_base_at_every_workgroup_shape(task, arms, wpb, n):
    opts = {"waves_per_block": wpb, "export_contacts": 1}
    generic = _run(task, arms, n, dict(opts, phys_specialised=0))
    spec = _run(task, arms, n, dict(opts, phys_specialised=2))
    _assert_identical(generic, spec, f"{task}_{arms}arms N={n} wpb={wpb}")
    # (not a trivial agreement: the envs moved, and differently from each other)
    assert np.abs(generic[-1][1]).max() > 0
    if n > 1:
        assert not np.array_equal(generic[-1][0][0], generic[-1][0][1])


# option -> (value off the default the kernels are compiled for, the default of an f32 handle)
OFF_DEFAULT = {"solver": (0, 1), "noslip_iters": (5, 3), "newton_early_exit": (0, 1), "qcqp_tridiag": (0, 2)}


@pytest.mark.parametrize("option", list(OFF_DEFAULT))
def test_option_off_default_falls_back_to_the_generic_kernel(option):
    from av_aloha_amd import _ffi
    from av_aloha_amd.sim import BatchedSim
    value, default = OFF_DEFAULT[option]
    task, arms, n = "slot_insertion", 3, 4
    ids = np.arange(n)
    md = model_dict(task, arms)
    sim = BatchedSim(task, arms, n, options={option: value})
    sim.reset(W.object_poses(task, ids, 1000))
    acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], ids, 2, sim.nj, 1000)
    before = [x.copy() for x in sim.get_state()] + [sim.get_latch()]
    sim.set_option("phys_specialised", 2)
    with pytest.raises(_ffi.AvsimError) as ei:
        sim.step(acts[0])
    assert "phys_specialised" in str(ei.value) and "generic" in str(ei.value), str(ei.value)
    for what, x, y in zip(("qpos", "qvel", "ctrl", "warmstart", "latch"), before, list(sim.get_state()) + [sim.get_latch()]):
        assert np.array_equal(x, y), f"{option} = {value}: the refused step changed {what}"
    # back at the default the handle takes its model's kernel again: "require" does not object
    sim.set_option(option, default)
    sim.step(acts[0])
    sim.step(acts[1])
    assert np.isfinite(sim.get_state()[0]).all() and not np.array_equal(sim.get_state()[0], before[0])
    sim.close()
    # phys_specialised = 1 with the option off its default runs, on the generic kernel: equal to 0 with the same option
    o = {option: value}
    _assert_identical(_run(task, arms, n, dict(o, phys_specialised=0)), _run(task, arms, n, dict(o, phys_specialised=1)), f"{option} = {value}")


def test_launches_without_substeps_take_the_model_kernel_too():
    """reset and the depth renderer's pose pass are k_phys launches with nsub = 0."""
    from av_aloha_amd.sim import BatchedSim
    task, arms, n = "slot_insertion", 3, 4
    ids = np.arange(n)
    md = model_dict(task, arms)
    acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], ids, 1, 21, 1000)
    out = {}
    for mode in (0, 2):
        sim = BatchedSim(task, arms, n, options={"phys_specialised": mode})
        sim.reset(W.object_poses(task, ids, 1000))
        after_reset = [x.copy() for x in sim.get_state()]
        sim.step(acts[0])
        depth = sim.render_depth(["overhead_cam"], 32, 32)
        out[mode] = after_reset + [x.copy() for x in sim.get_state()] + [depth, sim.diag()]
        sim.close()
    names = ["qpos after reset", "qvel after reset", "ctrl after reset", "warmstart after reset", "qpos", "qvel", "ctrl", "warmstart", "depth", "diag"]
    for name, x, y in zip(names, out[0], out[2]):
        assert x.shape == y.shape and np.array_equal(x, y), f"{name} differs between phys_specialised = 0 and 2"
    depth = out[2][8]
    assert depth.shape == (n, 1, 32, 32) and np.isfinite(depth).all() and depth.max() > depth.min()
    assert not np.array_equal(out[2][4], out[2][0])      # the step moved the envs
