"""The numpy front (BatchedSim) and the torch front (DeviceImageOps / VecEnv) of the nine device image calls hand libavsim the same call:
the same entry point, the same scalars and the same bytes in every array the library reads on the host.  No GPU: a recording stand-in
takes the library's place, and the torch front runs on CPU tensors with its stream binding switched off."""
import ctypes

import numpy as np
import pytest
import torch

from av_aloha_amd import _ffi, imgaug
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import VecEnv

# Per entry point: {argument position: bytes the library reads there}, as a function of the argument list.  These are the HOST arrays of
# include/avsim.h plus the small arrays that follow the I/O mode (index, values, lut), which a CPU tensor lets the test read as well.  Every
# other pointer (pixels in, results out) is compared as given / not given, every other argument as a value.
READ = {
    "avsim_compose": lambda a: {11: 24 * a[12]},
    "avsim_compose_label": lambda a: {6: 16 * a[7], 9: 8 * a[7]},
    "avsim_image_stats": lambda a: {3: 4 * a[4]},
    "avsim_image_prep": lambda a: {6: 3072 * a[7], 8: 4 * a[10], 9: 12 * a[10], 11: 4 * a[10]},
    "avsim_image_jitter": lambda a: {5: 16 * a[8], 6: 20 * a[8], 7: 4 * a[8], 9: 24},
    "avsim_image_augment": lambda a: {5: 16 * a[10], 6: 20 * a[10], 7: 24 * a[10], 9: 4 * a[10], 11: 24},
    "avsim_image_resize": lambda a: {6: 20 * a[9], 7: 16 * a[9], 8: 4 * a[9], 11: 12, 12: 24},
    "avsim_camera_poses": lambda a: {1: 4 * a[2]},
    "avsim_point_cloud": lambda a: {1: 4 * a[2], 6: 24},
    "avsim_render_depth": lambda a: {1: 4 * a[2]},
}
POINTERS = {"avsim_compose": (1, 6), "avsim_compose_label": (1,), "avsim_image_stats": (1, 7), "avsim_image_prep": (1, 14),
            "avsim_image_jitter": (1, 12), "avsim_image_augment": (1, 14), "avsim_image_resize": (1, 15), "avsim_camera_poses": (3,),
            "avsim_point_cloud": (5, 9, 10, 11), "avsim_render_depth": (5,)}
MESSAGE = "refused: a crop outside the source"


class RecordingLib:
    """Every avsim_* attribute is a function that appends (name, arguments) to .calls -- host arrays as their bytes, the other pointers as
    True / None -- and returns .rc."""

    def __init__(self):
        self.calls, self.rc = [], 0

    def avsim_last_error(self, h):
        return MESSAGE.encode()

    def __getattr__(self, name):
        if not name.startswith("avsim_"):
            raise AttributeError(name)

        def call(*args):
            a = list(args)
            for i, nbytes in READ[name](args).items():
                a[i] = None if args[i] is None else ctypes.string_at(args[i], nbytes)
            for i in POINTERS[name]:
                a[i] = None if args[i] is None else True
            self.calls.append((name, tuple(a)))
            return self.rc
        return call


class StandInHandle:
    h, num_envs = 1234, 2

    def __init__(self, L):
        self.L = L

    def check(self, rc):
        if rc != 0:
            raise _ffi.AvsimError(f"libavsim error {rc}")


class TorchFront(VecEnv):
    def _bind_stream(self):
        pass


def fronts():
    """(numpy owner, its library), (torch owner, its library): no GPU, no libavsim."""
    ln, lt = RecordingLib(), RecordingLib()
    manifest = {"camera_names": ["wrist", "overhead", "worms_eye"]}
    sim = object.__new__(BatchedSim)
    sim.h, sim.N, sim.manifest = StandInHandle(ln), 2, manifest
    env = object.__new__(TorchFront)
    env.torch, env.device, env._stream = torch, torch.device("cpu"), None
    env.h, env.L, env.num_envs, env.manifest = StandInHandle(lt), lt, 2, manifest
    return (sim, ln), (env, lt)


RNG = np.random.default_rng(7)
SRC = RNG.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)                   # 2 source images of 5 x 7
SRC_F32 = RNG.random((2, 3, 5, 7), dtype=np.float32)
OUT_HW, SRC_INDEX, NOUT = (3, 4), (1, 0, 1), 3                             # 3 outputs of 3 x 4
BOX = [[0, 0, 0], [3, 2, 1], [1, 1, 0]]                                    # (x0, y0, flip): one output flipped
LUT = RNG.random((2, 3, 256), dtype=np.float32)
LUT_INDEX = (0, 1, 0)                                                      # one table index non-zero
PARAMS = np.zeros(NOUT, dtype=imgaug.PARAMS_DTYPE)
PARAMS["x0"], PARAMS["y0"], PARAMS["flip"], PARAMS["mask"] = (0, 3, 1), (0, 2, 1), (0, 1, 0), (1, 34, 0)
PARAMS["factor"] = RNG.uniform(0.8, 1.2, (NOUT, 5))
MATRIX = np.stack([imgaug.affine_matrix(10.0 * i, tx=0.5 * i, scale=1.0 + 0.1 * i) for i in range(NOUT)])
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SRC_BOX = [[0, 0, 7, 5, 0], [1, 1, 5, 3, 1], [2, 0, 4, 4, 0]]              # (x0, y0, w, h, flip)
DST = [[0, 0, 4, 3], [0, 1, 4, 2], [1, 0, 3, 3]]                           # (ox, oy, rw, rh)
FILL = (0.5, 0.25, 0.125)
PLACES = [[0, 1, 0, 0, 4, 3], [1, 0, 2, 1, 4, 3], [2, 1, 4, 3, 4, 3]]      # (out image, src image, x0, y0, w, h) on 6 x 8 canvases
WHERE = [[0, 0, 0, 1], [1, 2, 1, 1], [2, 1, 0, 2]]                         # (out image, x, y, scale)
VALUES = np.array([3, 14, 159], dtype=np.int64)
INDEX = np.array([1, 0, 1], dtype=np.int32)
CAMERAS = ("worms_eye", 0)                                                 # a 2-camera id list, by name and by index
BOUNDS = (-0.5, -0.4, 0.0, 0.5, 0.4, 0.6)
DEPTH = RNG.random((2, 2, 3, 4), dtype=np.float32)

# call -> (the call on owner o, whose arrays are dev(numpy array); shape, numpy dtype and torch dtype of every result)
F32, U8 = (np.float32, torch.float32), (np.uint8, torch.uint8)
CALLS = {
    "compose": (lambda o, dev: o.compose(dev(SRC), PLACES, canvas_hw=(6, 8)), [((3, 6, 8, 3), *U8)]),
    "compose_clear_f32": (lambda o, dev: o.compose(dev(SRC_F32), PLACES[:2], out=dev(np.zeros((2, 3, 6, 8), np.float32)), clear=0x102030),
                          [((2, 3, 6, 8), *F32)]),
    "compose_label": (lambda o, dev: o.compose_label(dev(np.zeros((3, 6, 8, 3), np.uint8)), WHERE, prefix="ep ", values=dev(VALUES), rgb=0x00FF80),
                      [((3, 6, 8, 3), *U8)]),
    "compose_label_prefix": (lambda o, dev: o.compose_label(dev(np.zeros((3, 3, 6, 8), np.float32)), WHERE[:1], prefix="done"), [((3, 3, 6, 8), *F32)]),
    "image_stats": (lambda o, dev: o.image_stats(dev(SRC)), [((2, 3, 4), np.uint64, torch.int64)]),
    "image_stats_index": (lambda o, dev: o.image_stats(dev(SRC_F32), index=dev(INDEX)), [((3, 3, 4), np.uint64, torch.int64)]),
    "prep_images": (lambda o, dev: o.prep_images(dev(SRC), dev(LUT), BOX, OUT_HW, lut_index=LUT_INDEX, src_index=SRC_INDEX), [((3, 3, 3, 4), *F32)]),
    "prep_images_defaults": (lambda o, dev: o.prep_images(dev(SRC_F32), dev(LUT[0]), BOX[:2], OUT_HW), [((2, 3, 3, 4), *F32)]),
    "jitter_images": (lambda o, dev: o.jitter_images(dev(SRC), PARAMS, OUT_HW, mean=MEAN, std=STD, src_index=SRC_INDEX), [((3, 3, 3, 4), *F32)]),
    "jitter_images_pair": (lambda o, dev: o.jitter_images(dev(SRC), imgaug.split_params(PARAMS[:2]), OUT_HW), [((2, 3, 3, 4), *F32)]),
    "augment_images": (lambda o, dev: o.augment_images(dev(SRC), PARAMS, MATRIX, OUT_HW, interp=1, mean=MEAN, std=STD, src_index=SRC_INDEX),
                       [((3, 3, 3, 4), *F32)]),
    "augment_images_no_matrix": (lambda o, dev: o.augment_images(dev(SRC), PARAMS[:2], None, OUT_HW), [((2, 3, 3, 4), *F32)]),
    "resize_images": (lambda o, dev: o.resize_images(dev(SRC), SRC_BOX, DST, OUT_HW, antialias=False, fill=FILL, mean=MEAN, std=STD, src_index=SRC_INDEX),
                      [((3, 3, 3, 4), *F32)]),
    "resize_images_defaults": (lambda o, dev: o.resize_images(dev(SRC_F32), SRC_BOX[:2], DST[:2], OUT_HW), [((2, 3, 3, 4), *F32)]),
    "camera_poses": (lambda o, dev: o.camera_poses(CAMERAS), [((2, 2, 16), *F32)]),
    "point_cloud": (lambda o, dev: o.point_cloud(CAMERAS, 3, 4, BOUNDS, 5),
                    [((2, 5, 3), *F32), ((2, 5), np.int32, torch.int32), ((2, 2), np.int32, torch.int32)]),
    "point_cloud_depth": (lambda o, dev: o.point_cloud(CAMERAS, 3, 4, BOUNDS, 5, max_depth=1.5, depth=dev(DEPTH)),
                          [((2, 5, 3), *F32), ((2, 5), np.int32, torch.int32), ((2, 2), np.int32, torch.int32)]),
}
ENTRY = {"compose": "avsim_compose", "compose_label": "avsim_compose_label", "image_stats": "avsim_image_stats", "prep_images": "avsim_image_prep",
         "jitter_images": "avsim_image_jitter", "augment_images": "avsim_image_augment", "resize_images": "avsim_image_resize",
         "camera_poses": "avsim_camera_poses", "point_cloud": "avsim_point_cloud"}
NINE = tuple(ENTRY)


def as_numpy(a):
    return a


def as_torch(a):
    return torch.from_numpy(np.array(a))          # (a copy: the fronts share no memory)


def entry_of(case):
    return ENTRY[max((c for c in ENTRY if case.startswith(c)), key=len)]


def test_the_cases_cover_the_nine_calls():
    assert {entry_of(c) for c in CALLS} == set(ENTRY.values()) and len(NINE) == 9 and all(c in CALLS for c in NINE)


@pytest.mark.parametrize("case", CALLS)
def test_both_fronts_make_the_same_call(case):
    """The entry point, every scalar and the bytes of every host array agree between the fronts, and each front returns its own kind of
    array in the documented shape and type."""
    run, results = CALLS[case]
    (sim, ln), (env, lt) = fronts()
    rn, rt = run(sim, as_numpy), run(env, as_torch)
    assert ln.calls[-1][0] == entry_of(case)
    assert [c[0] for c in ln.calls] == [c[0] for c in lt.calls]
    for (name, an), (_, at) in zip(ln.calls, lt.calls):
        assert len(an) == len(at)
        for i, (x, y) in enumerate(zip(an, at)):
            assert type(x) is type(y) and x == y, f"{name}: argument {i}: {x!r} (numpy front) != {y!r} (torch front)"
    rn, rt = (rn if isinstance(rn, tuple) else (rn,)), (rt if isinstance(rt, tuple) else (rt,))
    assert len(rn) == len(rt) == len(results)
    for a, t, (shape, ndt, tdt) in zip(rn, rt, results):
        assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == ndt and a.flags.c_contiguous
        assert isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == tdt and t.is_contiguous() and t.device == env.device


def test_point_cloud_renders_the_depth_it_is_not_given():
    (sim, ln), (env, lt) = fronts()
    for o, L, dev in ((sim, ln, as_numpy), (env, lt, as_torch)):
        CALLS["point_cloud"][0](o, dev)
        assert [c[0] for c in L.calls] == ["avsim_render_depth", "avsim_point_cloud"]
        assert L.calls[0][1][2:5] == (2, 3, 4) and L.calls[1][1][5] is True
        L.calls.clear()
        CALLS["point_cloud_depth"][0](o, dev)
        assert [c[0] for c in L.calls] == ["avsim_point_cloud"] and L.calls[0][1][7] == 1.5


def test_the_host_arrays_are_what_was_passed():
    """The bytes compared above are the caller's values in the library's types (not, say, two equally wrong conversions)."""
    (sim, ln), _ = fronts()
    CALLS["prep_images"][0](sim, as_numpy)
    a = ln.calls[-1][1]
    assert a[2:6] == (0, 2, 5, 7) and a[7] == 2 and a[10] == 3 and a[12:14] == OUT_HW
    assert a[6] == LUT.tobytes() and a[8] == np.array(LUT_INDEX, np.int32).tobytes() and a[9] == np.array(BOX, np.int32).tobytes()
    assert a[11] == np.array(SRC_INDEX, np.int32).tobytes()
    CALLS["point_cloud_depth"][0](sim, as_numpy)
    a = ln.calls[-1][1]
    assert a[1] == np.array([2, 0], np.int32).tobytes() and a[6] == np.array(BOUNDS, np.float32).tobytes() and a[2:5] == (2, 3, 4) and a[8] == 5
    CALLS["augment_images"][0](sim, as_numpy)
    a = ln.calls[-1][1]
    assert a[7] == MATRIX.astype(np.float32).tobytes() and a[8] == 1 and a[11] == np.array([MEAN, STD], np.float32).tobytes()
    assert a[5] == np.array([[0, 0, 0, 1], [3, 2, 1, 34], [1, 1, 0, 0]], np.int32).tobytes()


@pytest.mark.parametrize("call", NINE)
def test_status_of_the_library(call):
    """AVSIM_EINVAL (-1) is a ValueError with the library's message, any other failure an AvsimError, on both fronts."""
    run = CALLS[call + "_depth" if call == "point_cloud" else call][0]        # (with the depth given: the one library call is the cloud's)
    for (o, L), dev in zip(fronts(), (as_numpy, as_torch)):
        L.rc = -1
        with pytest.raises(ValueError, match=MESSAGE):
            run(o, dev)
        L.rc = -3
        with pytest.raises(_ffi.AvsimError):
            run(o, dev)


WRONG_OUT = {
    "prep_images": lambda o, dev, out: o.prep_images(dev(SRC), dev(LUT), BOX, OUT_HW, out=out),
    "jitter_images": lambda o, dev, out: o.jitter_images(dev(SRC), PARAMS, OUT_HW, out=out),
    "augment_images": lambda o, dev, out: o.augment_images(dev(SRC), PARAMS, MATRIX, OUT_HW, out=out),
    "resize_images": lambda o, dev, out: o.resize_images(dev(SRC), SRC_BOX, DST, OUT_HW, out=out),
}


@pytest.mark.parametrize("call", WRONG_OUT)
@pytest.mark.parametrize("shape, dtype", [((3, 3, 4, 3), np.float32), ((2, 3, 3, 4), np.float32), ((3, 3, 3, 4), np.float64)])
def test_a_wrong_out_is_refused_before_the_library_sees_it(call, shape, dtype):
    (sim, ln), (env, lt) = fronts()
    with pytest.raises(ValueError):
        WRONG_OUT[call](sim, as_numpy, np.zeros(shape, dtype))
    with pytest.raises(AssertionError):
        WRONG_OUT[call](env, as_torch, as_torch(np.zeros(shape, dtype)))
    with pytest.raises(ValueError):
        WRONG_OUT[call](sim, as_numpy, np.zeros((3, 3, 3, 8), np.float32)[:, :, :, ::2])          # not contiguous
    with pytest.raises(AssertionError):
        WRONG_OUT[call](env, as_torch, torch.zeros((3, 3, 3, 8))[:, :, :, ::2])
    assert not ln.calls and not lt.calls


def test_a_wrong_canvas_or_image_is_refused_before_the_library_sees_it():
    (sim, ln), (env, lt) = fronts()
    with pytest.raises(ValueError):
        sim.compose(SRC, PLACES, out=np.zeros((6, 8, 3), np.uint8))
    with pytest.raises(AssertionError):
        env.compose(as_torch(SRC), PLACES, out=torch.zeros((6, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        sim.compose_label([[0, 0, 0]], WHERE)                                # the canvas is written in place: an array, not a list
    with pytest.raises(AssertionError):
        env.compose_label(np.zeros((3, 6, 8, 3), np.uint8), WHERE)           # a numpy canvas on the torch front
    for call in ("jitter_images", "augment_images"):                          # img of the wrong type
        args = (PARAMS, OUT_HW) if call == "jitter_images" else (PARAMS, MATRIX, OUT_HW)
        with pytest.raises(ValueError):
            getattr(sim, call)(SRC_F32, *args)
        with pytest.raises(AssertionError):
            getattr(env, call)(as_torch(SRC_F32), *args)
    with pytest.raises(ValueError):
        sim.point_cloud(CAMERAS, 3, 4, BOUNDS, 5, depth=DEPTH[:, :1])
    with pytest.raises(AssertionError):
        env.point_cloud(CAMERAS, 3, 4, BOUNDS, 5, depth=as_torch(DEPTH[:, :1]))
    assert not ln.calls and not lt.calls


def test_what_differs_between_the_fronts():
    """The numpy front converts what it is given; the torch front takes tensors as they are and says so."""
    (sim, ln), (env, lt) = fronts()
    r = sim.prep_images(np.asfortranarray(SRC), LUT.reshape(-1).tolist(), BOX, OUT_HW)        # not C-contiguous; a flat list for the tables
    assert r.shape == (3, 3, 3, 4) and ln.calls[-1][1][6] == LUT.tobytes() and ln.calls[-1][1][7] == 2
    sim.image_stats(SRC[:, :, ::-1])                                                          # not contiguous
    with pytest.raises(AssertionError):
        env.image_stats(as_torch(SRC).flip(2)[:, :, ::2])
    with pytest.raises(AssertionError):
        env.prep_images(as_torch(SRC), as_torch(LUT.astype(np.float64)), BOX, OUT_HW)
    sim.compose_label(np.zeros((3, 6, 8, 3), np.uint8), WHERE, values=[3, 14, 159])
    assert ln.calls[-1][1][9] == VALUES.tobytes()
    with pytest.raises(AssertionError):
        env.compose_label(torch.zeros((3, 6, 8, 3), dtype=torch.uint8), WHERE, values=as_torch(VALUES.astype(np.int32)))
    with pytest.raises(ValueError, match="index outside"):                                   # the numpy front refuses, the torch front clamps
        sim.image_stats(SRC, index=[0, 2])
    env.image_stats(as_torch(SRC), index=torch.tensor([0, 2, -1], dtype=torch.int32))
    assert lt.calls[-1][1][3] == np.array([0, 1, 0], np.int32).tobytes()
    out = torch.zeros((2, 3, 4), dtype=torch.int64)
    assert env.image_stats(as_torch(SRC), out=out) is out
    c = env.compose(as_torch(SRC), PLACES, canvas_hw=(6, 8), fmt="lerobot")                   # fmt: the format of a new canvas
    assert tuple(c.shape) == (3, 3, 6, 8) and c.dtype == torch.float32 and lt.calls[-1][1][7] == 1 and lt.calls[-1][1][13:] == (1, 0)
