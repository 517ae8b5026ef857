"""virtual_views of the numpy front (BatchedSim) and of the torch front (DeviceImageOps / VecEnv) hand libavsim the same avsim_virtual_views
call, render first exactly what they were not given, and refuse a wrong depth, rgb, out or index before the library sees it.  No GPU: the
recording stand-in of test_image_fronts_host.py, with this call's host arrays."""
import ctypes

import numpy as np
import pytest
import torch

from av_aloha_amd import _ffi
from av_aloha_amd.sim import BatchedSim
from test_image_fronts_host import BOUNDS, CAMERAS, DEPTH, MESSAGE, StandInHandle, TorchFront, as_numpy, as_torch

# {argument position: bytes the library reads there on the host}; the other pointers are compared as given / not given
READ = {"avsim_virtual_views": lambda a: {1: 4 * a[2], 7: 24, 9: 4 * a[10], 11: 8}, "avsim_render_depth": lambda a: {1: 4 * a[2]}, "avsim_render_rgb": lambda a: {1: 4 * a[2]},
        "avsim_set_option": lambda a: {}}
POINTERS = {"avsim_virtual_views": (5, 6, 13, 14), "avsim_render_depth": (5,), "avsim_render_rgb": (5,), "avsim_set_option": ()}
RGB = np.random.default_rng(9).integers(0, 256, (2, 2, 3, 4, 3), dtype=np.uint8)
VIEWS = ["+z", "-x", 2]
SIZE = (5, 6)


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


ARGS = (CAMERAS, 3, 4, BOUNDS, VIEWS, SIZE)
CASES = {
    "nothing given": (lambda o, dev: o.virtual_views(*ARGS), ["avsim_render_depth", "avsim_virtual_views"], False),
    "nothing given, colour": (lambda o, dev: o.virtual_views(*ARGS, colour=True), ["avsim_render_depth", "avsim_set_option", "avsim_render_rgb", "avsim_virtual_views"], True),
    "depth given": (lambda o, dev: o.virtual_views(*ARGS, radius=3, max_depth=1.5, depth=dev(DEPTH)), ["avsim_virtual_views"], False),
    "depth given, colour": (lambda o, dev: o.virtual_views(*ARGS, depth=dev(DEPTH), colour=True), ["avsim_set_option", "avsim_render_rgb", "avsim_virtual_views"], True),
    "rgb given": (lambda o, dev: o.virtual_views(*ARGS, rgb=dev(RGB)), ["avsim_render_depth", "avsim_virtual_views"], True),
    "both given": (lambda o, dev: o.virtual_views(CAMERAS, 3, 4, BOUNDS, "-z", 7, depth=dev(DEPTH), rgb=dev(RGB), colour=True), ["avsim_virtual_views"], True),
}


@pytest.mark.parametrize("case", CASES)
def test_both_fronts_make_the_same_calls(case):
    """The renders precede the call exactly when depth or rgb is missing; entry points, scalars and the bytes of the host arrays agree
    between the fronts; each front returns its own kind of arrays, float32 [N, V, VH, VW, 8] and int32 [N, V, VH, VW]."""
    run, names, has_rgb = CASES[case]
    (sim, ln, _), (env, lt, _) = fronts()
    rn, rt = run(sim, as_numpy), run(env, as_torch)
    assert [c[0] for c in ln.calls] == names == [c[0] for c in lt.calls]
    for (name, an), (_, at) in zip(ln.calls, lt.calls):
        assert len(an) == len(at)
        for i, (x, y) in enumerate(zip(an, at)):
            assert type(x) is type(y) and x == y, f"{name}: argument {i}: {x!r} (numpy front) != {y!r} (torch front)"
    a = ln.calls[-1][1]
    codes, size = ([5], (7, 7)) if case == "both given" else ([4, 1, 2], SIZE)
    assert len(a) == 15 and a[1] == np.array([2, 0], np.int32).tobytes() and a[2:5] == (2, 3, 4) and a[5] is True and a[6] is (True if has_rgb else None)
    assert a[7] == np.array(BOUNDS, np.float32).tobytes() and a[8] == (1.5 if case == "depth given" else 30.0)
    assert a[9] == np.array(codes, np.int32).tobytes() and a[10] == len(codes) and a[11] == np.array(size, np.int32).tobytes() and a[12] == (3 if case == "depth given" else 1)
    assert a[13] is True and a[14] is True
    for c in ln.calls[:-1]:
        if c[0] == "avsim_set_option":          # the call's own colour render is env-major
            assert c[1][1:] == (b"render_cam_major", 0.0)
            continue
        assert c[1][1] == np.array([2, 0], np.int32).tobytes() and c[1][2:5] == (2, 3, 4) and c[1][5] is True
    shape = (2, len(codes)) + size
    assert isinstance(rn, tuple) and isinstance(rt, tuple) and len(rn) == len(rt) == 2
    assert isinstance(rn[0], np.ndarray) and rn[0].shape == shape + (8,) and rn[0].dtype == np.float32 and rn[0].flags.c_contiguous
    assert isinstance(rn[1], np.ndarray) and rn[1].shape == shape and rn[1].dtype == np.int32 and rn[1].flags.c_contiguous
    assert isinstance(rt[0], torch.Tensor) and tuple(rt[0].shape) == shape + (8,) and rt[0].dtype == torch.float32 and rt[0].is_contiguous()
    assert isinstance(rt[1], torch.Tensor) and tuple(rt[1].shape) == shape and rt[1].dtype == torch.int32 and rt[1].is_contiguous()


def test_the_colour_render_is_env_major_and_the_owner_gets_its_layout_back():
    """An owner that keeps "render_cam_major" on (a VecEnv with `cameras`: _cam_major 1) has it switched off round the call's own colour
    render and on again before the views call -- also when the render fails; an rgb that is given touches no option."""
    for o, L, dev in fronts():
        o._cam_major = 1
        o.virtual_views(*ARGS, depth=dev(DEPTH), colour=True)
        assert [(c[0], c[1][1:] if c[0] == "avsim_set_option" else None) for c in L.calls] == [
            ("avsim_set_option", (b"render_cam_major", 0.0)), ("avsim_render_rgb", None), ("avsim_set_option", (b"render_cam_major", 1.0)), ("avsim_virtual_views", None)]
        L.calls.clear()
        o.virtual_views(*ARGS, depth=dev(DEPTH), rgb=dev(RGB), colour=True)
        assert [c[0] for c in L.calls] == ["avsim_virtual_views"]
        L.calls.clear()
        L.fail_on = "avsim_render_rgb"
        with pytest.raises(_ffi.AvsimError):
            o.virtual_views(*ARGS, depth=dev(DEPTH), colour=True)
        assert [c[0] for c in L.calls] == ["avsim_set_option", "avsim_render_rgb", "avsim_set_option"] and L.calls[-1][1][2] == 1.0


def test_channels_first_is_a_view():
    _, (env, lt, _) = fronts()
    out, index = torch.zeros((2, 3, 5, 6, 8)), torch.zeros((2, 3, 5, 6), dtype=torch.int32)
    v, i = env.virtual_views(*ARGS, depth=as_torch(DEPTH), out=out, index=index, channels_first=True)
    assert tuple(v.shape) == (2, 3, 8, 5, 6) and v.data_ptr() == out.data_ptr() and v.stride() == (720, 240, 1, 48, 8) and i is index
    flat = v.flatten(0, 1)          # the views of all envs as one channels_last batch for a 2-D network: still no copy
    assert tuple(flat.shape) == (6, 8, 5, 6) and flat.data_ptr() == out.data_ptr() and flat.is_contiguous(memory_format=torch.channels_last)
    o2, i2 = env.virtual_views(*ARGS, depth=as_torch(DEPTH), out=out, index=index)
    assert o2 is out and i2 is index


def test_status_of_the_library():
    for o, L, dev in fronts():
        L.rc = -1
        with pytest.raises(ValueError, match=MESSAGE):
            CASES["both given"][0](o, dev)
        L.rc = -3
        with pytest.raises(_ffi.AvsimError):
            CASES["both given"][0](o, dev)


def test_a_wrong_depth_rgb_out_or_index_is_refused_before_the_library_sees_it():
    (sim, ln, _), (env, lt, _) = fronts()
    f32, i32 = np.float32, np.int32
    wrong = [dict(depth=DEPTH[:, :1]), dict(depth=DEPTH, rgb=RGB[:, :1]), dict(depth=DEPTH, rgb=RGB[..., :2]),
             dict(depth=DEPTH, out=np.zeros((2, 3, 5, 6, 7), f32)), dict(depth=DEPTH, out=np.zeros((2, 3, 5, 6, 8), np.float64)),
             dict(depth=DEPTH, out=np.zeros((2, 3, 8, 5, 6), f32)), dict(depth=DEPTH, out=np.zeros((2, 2, 5, 6, 8), f32)),
             dict(depth=DEPTH, index=np.zeros((2, 3, 5, 6), np.int64)), dict(depth=DEPTH, index=np.zeros((2, 3, 6, 5), i32)), dict(depth=DEPTH, index=np.zeros((2, 3, 5, 6, 1), i32))]
    for kw in wrong:
        with pytest.raises(ValueError):
            sim.virtual_views(*ARGS, **kw)
        with pytest.raises(AssertionError):
            env.virtual_views(*ARGS, **{k: as_torch(v) for k, v in kw.items()})
    with pytest.raises(ValueError):          # not contiguous
        sim.virtual_views(*ARGS, depth=DEPTH, out=np.zeros((2, 3, 5, 6, 16), f32)[..., ::2])
    with pytest.raises(AssertionError):
        env.virtual_views(*ARGS, depth=as_torch(DEPTH), out=torch.zeros((2, 3, 5, 6, 16))[..., ::2])
    with pytest.raises(AssertionError):
        env.virtual_views(*ARGS, depth=as_torch(DEPTH), index=torch.zeros((2, 3, 5, 12), dtype=torch.int32)[..., ::2])
    with pytest.raises(AssertionError):
        env.virtual_views(*ARGS, depth=as_torch(DEPTH.astype(np.float64)))
    with pytest.raises(AssertionError):
        env.virtual_views(*ARGS, depth=as_torch(DEPTH), rgb=as_torch(RGB.astype(np.float32)))
    with pytest.raises(ValueError):          # the other front's kind of array
        sim.virtual_views(*ARGS, depth=DEPTH, out=torch.zeros((2, 3, 5, 6, 8)))
    with pytest.raises(AssertionError):
        env.virtual_views(*ARGS, depth=as_torch(DEPTH), index=np.zeros((2, 3, 5, 6), i32))
    for o, _, dev in fronts():          # views or a size that are none, before outputs of that size are made
        for views, size in (([], SIZE), ([0] * 7, SIZE), (["top"], SIZE), ([1.5], SIZE), (VIEWS, 0), (VIEWS, (1025, 2)), (VIEWS, (4, 3, 2)), (VIEWS, (4, -3))):
            with pytest.raises(ValueError):
                o.virtual_views(CAMERAS, 3, 4, BOUNDS, views, size, depth=dev(DEPTH))
        with pytest.raises(ValueError):
            o.virtual_views(CAMERAS, 3, 4, BOUNDS[:5], VIEWS, SIZE, depth=dev(DEPTH))
    assert not ln.calls and not lt.calls
