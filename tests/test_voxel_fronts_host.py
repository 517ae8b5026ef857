"""voxel_grid of the numpy front (BatchedSim) and of the torch front (DeviceImageOps / VecEnv) hand libavsim the same avsim_voxel_grid call,
render first exactly what they were not given, and refuse a wrong depth, rgb or out before the library sees it.  No GPU: the recording
stand-in of test_image_fronts_host.py, with this call's host arrays."""
import ctypes

import numpy as np
import pytest
import torch

from av_aloha_amd import _ffi
from av_aloha_amd.sim import BatchedSim
from test_image_fronts_host import BOUNDS, CAMERAS, DEPTH, MESSAGE, StandInHandle, TorchFront, as_numpy, as_torch

# {argument position: bytes the library reads there on the host}; the other pointers are compared as given / not given
READ = {"avsim_voxel_grid": lambda a: {1: 4 * a[2], 7: 24, 9: 12}, "avsim_render_depth": lambda a: {1: 4 * a[2]}, "avsim_render_rgb": lambda a: {1: 4 * a[2]},
        "avsim_set_option": lambda a: {}}
POINTERS = {"avsim_voxel_grid": (5, 6, 10), "avsim_render_depth": (5,), "avsim_render_rgb": (5,), "avsim_set_option": ()}
RGB = np.random.default_rng(8).integers(0, 256, (2, 2, 3, 4, 3), dtype=np.uint8)
GRID = (4, 3, 2)


class RecordingLib:
    def __init__(self):
        self.calls, self.rc, self.fail_on = [], 0, None

    def avsim_last_error(self, h):
        return MESSAGE.encode()

    def __getattr__(self, name):
        if name not in READ:
            raise AttributeError(name)

        def call(*args):
            a = list(args)
            for i, nbytes in READ[name](args).items():
                a[i] = None if args[i] is None else ctypes.string_at(args[i], nbytes)
            for i in POINTERS[name]:
                a[i] = None if args[i] is None else True
            self.calls.append((name, tuple(a)))
            if name == self.fail_on:
                return -3
            return self.rc if name != "avsim_set_option" else 0
        return call


def fronts():
    ln, lt = RecordingLib(), RecordingLib()
    manifest = {"camera_names": ["wrist", "overhead", "worms_eye"]}
    sim = object.__new__(BatchedSim)
    sim.h, sim.N, sim.manifest = StandInHandle(ln), 2, manifest
    env = object.__new__(TorchFront)
    env.torch, env.device, env._stream = torch, torch.device("cpu"), None
    env.h, env.L, env.num_envs, env.manifest = StandInHandle(lt), lt, 2, manifest
    return (sim, ln, as_numpy), (env, lt, as_torch)


CASES = {
    "nothing given": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID), ["avsim_render_depth", "avsim_voxel_grid"], False),
    "nothing given, colour": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, colour=True), ["avsim_render_depth", "avsim_set_option", "avsim_render_rgb", "avsim_voxel_grid"], True),
    "depth given": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, max_depth=1.5, depth=dev(DEPTH)), ["avsim_voxel_grid"], False),
    "depth given, colour": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=dev(DEPTH), colour=True), ["avsim_set_option", "avsim_render_rgb", "avsim_voxel_grid"], True),
    "rgb given": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, rgb=dev(RGB)), ["avsim_render_depth", "avsim_voxel_grid"], True),
    "both given": (lambda o, dev: o.voxel_grid(CAMERAS, 3, 4, BOUNDS, 5, depth=dev(DEPTH), rgb=dev(RGB), colour=True), ["avsim_voxel_grid"], True),
}


@pytest.mark.parametrize("case", CASES)
def test_both_fronts_make_the_same_calls(case):
    """The renders precede the call exactly when depth or rgb is missing; entry points, scalars and the bytes of the host arrays agree
    between the fronts; each front returns its own kind of array, float32 [N, gx, gy, gz, 8]."""
    run, names, has_rgb = CASES[case]
    (sim, ln, _), (env, lt, _) = fronts()
    rn, rt = run(sim, as_numpy), run(env, as_torch)
    assert [c[0] for c in ln.calls] == names == [c[0] for c in lt.calls]
    for (name, an), (_, at) in zip(ln.calls, lt.calls):
        assert len(an) == len(at)
        for i, (x, y) in enumerate(zip(an, at)):
            assert type(x) is type(y) and x == y, f"{name}: argument {i}: {x!r} (numpy front) != {y!r} (torch front)"
    a = ln.calls[-1][1]
    g = (5, 5, 5) if case == "both given" else GRID
    assert a[1] == np.array([2, 0], np.int32).tobytes() and a[2:5] == (2, 3, 4) and a[5] is True and a[6] is (True if has_rgb else None)
    assert a[7] == np.array(BOUNDS, np.float32).tobytes() and a[8] == (1.5 if case == "depth given" else 30.0) and a[9] == np.array(g, np.int32).tobytes() and a[10] is True
    for c in ln.calls[:-1]:
        if c[0] == "avsim_set_option":          # the grid's own colour render is env-major
            assert c[1][1:] == (b"render_cam_major", 0.0)
            continue
        assert c[1][1] == np.array([2, 0], np.int32).tobytes() and c[1][2:5] == (2, 3, 4) and c[1][5] is True
    shape = (2,) + g + (8,)
    assert isinstance(rn, np.ndarray) and rn.shape == shape and rn.dtype == np.float32 and rn.flags.c_contiguous
    assert isinstance(rt, torch.Tensor) and tuple(rt.shape) == shape and rt.dtype == torch.float32 and rt.is_contiguous()


def test_the_colour_render_is_env_major_and_the_owner_gets_its_layout_back():
    """An owner that keeps "render_cam_major" on (a VecEnv with `cameras`: _cam_major 1) has it switched off round voxel_grid's own colour
    render and on again before the grid call -- also when the render fails; an rgb that is given touches no option."""
    for o, L, dev in fronts():
        o._cam_major = 1
        o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=dev(DEPTH), colour=True)
        assert [(c[0], c[1][1:] if c[0] == "avsim_set_option" else None) for c in L.calls] == [
            ("avsim_set_option", (b"render_cam_major", 0.0)), ("avsim_render_rgb", None), ("avsim_set_option", (b"render_cam_major", 1.0)), ("avsim_voxel_grid", None)]
        L.calls.clear()
        o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=dev(DEPTH), rgb=dev(RGB), colour=True)
        assert [c[0] for c in L.calls] == ["avsim_voxel_grid"]
        L.calls.clear()
        L.fail_on = "avsim_render_rgb"
        with pytest.raises(_ffi.AvsimError):
            o.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=dev(DEPTH), colour=True)
        assert [c[0] for c in L.calls] == ["avsim_set_option", "avsim_render_rgb", "avsim_set_option"] and L.calls[-1][1][2] == 1.0


def test_channels_first_is_a_view():
    _, (env, lt, _) = fronts()
    out = torch.zeros((2, 4, 3, 2, 8))
    v = env.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=as_torch(DEPTH), out=out, channels_first=True)
    assert tuple(v.shape) == (2, 8, 4, 3, 2) and v.data_ptr() == out.data_ptr() and v.stride() == (192, 1, 48, 16, 8)
    assert v.is_contiguous(memory_format=torch.channels_last_3d)
    assert env.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=as_torch(DEPTH), out=out) is out


def test_status_of_the_library():
    for o, L, dev in fronts():
        L.rc = -1
        with pytest.raises(ValueError, match=MESSAGE):
            CASES["both given"][0](o, dev)
        L.rc = -3
        with pytest.raises(_ffi.AvsimError):
            CASES["both given"][0](o, dev)


def test_a_wrong_depth_rgb_or_out_is_refused_before_the_library_sees_it():
    (sim, ln, _), (env, lt, _) = fronts()
    wrong = [dict(depth=DEPTH[:, :1]), dict(depth=DEPTH, rgb=RGB[:, :1]), dict(depth=DEPTH, rgb=RGB[..., :2]),
             dict(depth=DEPTH, out=np.zeros((2, 4, 3, 2, 7), np.float32)), dict(depth=DEPTH, out=np.zeros((2, 4, 3, 2, 8), np.float64)),
             dict(depth=DEPTH, out=np.zeros((2, 4, 3, 2, 16), np.float32)[..., ::2]), dict(depth=DEPTH, out=np.zeros((2, 8, 4, 3, 2), np.float32))]
    for kw in wrong:
        with pytest.raises(ValueError):
            sim.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, **kw)
        with pytest.raises(AssertionError):
            env.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, **{k: as_torch(v) if k != "out" or v.flags.c_contiguous else torch.zeros((2, 4, 3, 2, 16))[..., ::2] for k, v in kw.items()})
    with pytest.raises(AssertionError):
        env.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=as_torch(DEPTH.astype(np.float64)))
    with pytest.raises(AssertionError):
        env.voxel_grid(CAMERAS, 3, 4, BOUNDS, GRID, depth=as_torch(DEPTH), rgb=as_torch(RGB.astype(np.float32)))
    for o, _, dev in fronts():          # a grid that is no grid, before an output of that size is made
        for grid in ((4, 3), 0, (257, 1, 1), (129, 128, 128), (4, 3, -2)):
            with pytest.raises(ValueError):
                o.voxel_grid(CAMERAS, 3, 4, BOUNDS, grid, depth=dev(DEPTH))
        with pytest.raises(ValueError):
            o.voxel_grid(CAMERAS, 3, 4, BOUNDS[:5], GRID, depth=dev(DEPTH))
    assert not ln.calls and not lt.calls
