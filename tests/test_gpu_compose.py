"""The device's composer (avsim_compose / avsim_compose_label, csrc/avsim_compose.hip.h) against its specification, av_aloha_amd/compose.py:
equal byte for byte through a host-pointer handle and a device handle, in all four format combinations -- the coefficients come from the
host and the device does integer arithmetic only, so there is no tolerance.  Then what the library refuses, the labels, and the layers
above the C calls: VecEnv.compose, harness.visualize_episode on the device against its host path, evaluate_vec's grid video.  (That the
specification is Pillow's bilinear resize is tests/test_compose_host.py's subject.)"""
import os

import numpy as np
import pytest

from av_aloha_amd import compose, harness, jpeg, mjpeg
from av_aloha_amd.vec_env import make_vec
from avsim_test_util import noise
from gpu_util import torch as T
from gpu_util import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
GUARD = 4096
FILL = 0xA5

# (source H, W) -> (rectangle h, w): the smallest shapes at which the kernel can go wrong
CASES = {"17x23-5x7": ((17, 23), (5, 7)),            # taps clipped at both edges, a ratio that is no integer
         "17x23-40x51": ((17, 23), (40, 51)),        # enlarging
         "33x65-32x64": ((33, 65), (32, 64)),        # almost a copy: two taps everywhere
         "9x9-1x1": ((9, 9), (1, 1)),
         "16x16-16x16": ((16, 16), (16, 16)),        # an exact copy, both passes skipped
         "64x48-4x3": ((64, 48), (4, 3)),            # ratio 16: the most taps
         "48x330-24x165": ((48, 330), (24, 165)),    # three column tiles, three row tiles that share source rows
         "64x48-64x20": ((64, 48), (64, 20)),        # the vertical pass skipped
         "64x48-30x48": ((64, 48), (30, 48))}        # the horizontal pass skipped


def to_f32(u8_nhwc):
    """u8 [n, H, W, 3] -> float32 [n, 3, H, W] = u8 / 255, the bits of avsim_render_rgb_f32 (and (int)(v * 255 + 0.5f) gives the u8 back)."""
    return (T.from_numpy(np.ascontiguousarray(u8_nhwc)).permute(0, 3, 1, 2).float() / 255).contiguous().numpy()


def call_host(sim, src, canvas, places, clear=None):
    """avsim_compose through the host-pointer handle, the formats taken from the arrays -> the return code (canvas written in place)."""
    sf, df = int(src.dtype == np.float32), int(canvas.dtype == np.float32)
    n, H, W = (src.shape[0], src.shape[2], src.shape[3]) if sf else src.shape[:3]
    no, CH, CW = (canvas.shape[0], canvas.shape[2], canvas.shape[3]) if df else canvas.shape[:3]
    p = np.ascontiguousarray(places, dtype=np.int32).reshape(-1, 6)
    return sim.h.L.avsim_compose(sim.h.h, src.ctypes.data, sf, n, H, W, canvas.ctypes.data, df, no, CH, CW, p.ctypes.data, len(p),
                                 0 if clear is None else 1, clear or 0)


def call_device(dev, src, canvas, places, clear=None):
    """The same through the device handle: src / canvas are torch tensors on the device."""
    h, _ = dev
    sf, df = int(src.dtype == T.float32), int(canvas.dtype == T.float32)
    n, H, W = (src.shape[0], src.shape[2], src.shape[3]) if sf else src.shape[:3]
    no, CH, CW = (canvas.shape[0], canvas.shape[2], canvas.shape[3]) if df else canvas.shape[:3]
    p = np.ascontiguousarray(places, dtype=np.int32).reshape(-1, 6)
    return h.L.avsim_compose(h.h, src.data_ptr(), sf, n, H, W, canvas.data_ptr(), df, no, CH, CW, p.ctypes.data, len(p),
                             0 if clear is None else 1, clear or 0)


@pytest.mark.parametrize("case", list(CASES))
def test_compose_equals_the_reference(sim, dev, case):
    (H, W), (h, w) = CASES[case]
    src = noise((2, H, W, 3), 1)
    src[0, :, :, 0] = np.linspace(0, 255, W).astype(np.uint8)[None]            # one channel a ramp
    # a rectangle at an odd x0 (unaligned u8 stores), flush against the canvas's right and bottom edges, and a second one at the origin
    x0 = w + 5 + w % 2
    assert x0 % 2 == 1
    CH, CW = h + 3 + h, x0 + w
    places = [(1, 1, x0, h + 3, w, h), (0, 0, 0, 0, w, h)]
    base = noise((2, CH, CW, 3), 2)
    want = compose.compose_reference(base.copy(), src, places)
    assert not np.array_equal(want, base)
    want_f32 = to_f32(want)
    for sf in (0, 1):
        s = to_f32(src) if sf else src
        for df in (0, 1):
            c = to_f32(base) if df else base.copy()
            assert call_host(sim, s, c, places) == 0, (case, sf, df)
            if df:
                assert T.equal(T.from_numpy(c), T.from_numpy(want_f32)), (case, "host", sf, df)
            else:
                assert np.array_equal(c, want), (case, "host", sf, df, int(np.abs(c.astype(int) - want).max()))
            ts, tc = T.from_numpy(s).to(dev[1]), T.from_numpy(to_f32(base) if df else base.copy()).to(dev[1])
            assert call_device(dev, ts, tc, places) == 0, (case, sf, df)
            T.cuda.synchronize()
            if df:
                assert T.equal(tc.cpu(), T.from_numpy(want_f32)), (case, "device", sf, df)
            else:
                assert np.array_equal(tc.cpu().numpy(), want), (case, "device", sf, df)


def guarded(nbytes, offset=0):
    """A device byte buffer with GUARD bytes of FILL on either side of `nbytes` bytes that start `offset` bytes past a dword boundary
    (the allocation is aligned, GUARD a multiple of four)."""
    whole = T.full((GUARD + offset + nbytes + GUARD,), FILL, dtype=T.uint8, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + nbytes]


def guards_intact(whole, nbytes, offset=0):
    a = whole.cpu().numpy()
    return (a[:GUARD + offset] == FILL).all() and (a[GUARD + offset + nbytes:] == FILL).all()


@pytest.mark.parametrize("offset", [0, 1])             # a canvas that starts on a dword (the fill kernel's dword path) and one that does not
def test_grid_and_two_cameras_with_guards(dev, offset):
    # six distinct source images into a 2 x 3 grid in ONE call, cleared first
    src = np.stack([noise((17, 23, 3), 10 + i) for i in range(6)])
    rows, CH, CW = compose.layout_grid(6, 5, 7, cols=3)
    assert (CH, CW) == (10, 21)
    CW += 4                                             # a margin that keeps the background colour
    places = [(0, i, x0, y0, w, h) for i, (x0, y0, w, h) in enumerate(rows)]
    whole, flat = guarded(CH * CW * 3, offset)
    canvas = flat.view(1, CH, CW, 3)
    assert call_device(dev, T.from_numpy(src).to(dev[1]), canvas, places, clear=0x102030) == 0
    T.cuda.synchronize()
    want = np.empty((1, CH, CW, 3), np.uint8)
    want[:] = (0x10, 0x20, 0x30)
    compose.compose_reference(want, src, places)
    assert np.array_equal(canvas.cpu().numpy(), want)
    assert (canvas.cpu().numpy()[0, :, 21:] == (0x10, 0x20, 0x30)).all()
    assert guards_intact(whole, CH * CW * 3, offset)
    # two cameras of different sizes in two calls onto one canvas, `clear` on the first only; float32 planes this time
    cams = [noise((2, 24, 32, 3), 20), noise((2, 36, 48, 3), 21)]
    rows, CH, CW = compose.layout_row([(24, 32), (36, 48)])
    CH += 2
    whole, flat = guarded(2 * 3 * CH * CW * 4, 4 * offset)
    canvas = flat.view(T.float32).view(2, 3, CH, CW)
    want = np.empty((2, CH, CW, 3), np.uint8)
    want[:] = (200, 0, 7)
    for k, (cam, (x0, y0, w, h)) in enumerate(zip(cams, rows)):
        pl = [(i, i, x0, y0, w, h) for i in range(2)]
        assert call_device(dev, T.from_numpy(cam).to(dev[1]), canvas, pl, clear=0xC80007 if k == 0 else None) == 0
        compose.compose_reference(want, cam, pl)
    T.cuda.synchronize()
    assert T.equal(canvas.cpu(), T.from_numpy(to_f32(want)))
    assert (want[:, 24:] == (200, 0, 7)).all()
    assert guards_intact(whole, 2 * 3 * CH * CW * 4, 4 * offset)


def test_what_the_library_refuses(sim, dev):
    src = noise((2, 34, 34, 3), 3)
    base = noise((1, 20, 20, 3), 4)
    bad = {"outside the canvas": [(0, 0, 14, 0, 7, 5)],
           "overlap": [(0, 0, 0, 0, 7, 5), (0, 1, 6, 4, 7, 5)],
           "ratio 17": [(0, 0, 0, 0, 7, 2)],
           "source index nsrc": [(0, 2, 0, 0, 7, 5)],
           "output index nout": [(1, 0, 0, 0, 7, 5)],
           "zero width": [(0, 0, 0, 0, 0, 5)],
           "negative x0": [(0, 0, -1, 0, 7, 5)]}
    for name, places in bad.items():
        with pytest.raises(ValueError):
            compose.compose_reference(base.copy(), src, places)          # the specification refuses the same
        for clear in (None, 0x334455):
            c = base.copy()
            assert call_host(sim, src, c, places, clear) == -1, name
            assert np.array_equal(c, base), name
            tc = T.from_numpy(base.copy()).to(dev[1])
            assert call_device(dev, T.from_numpy(src).to(dev[1]), tc, places, clear) == -1, name
            T.cuda.synchronize()
            assert np.array_equal(tc.cpu().numpy(), base), name
    assert call_host(sim, src, base.copy(), bad["overlap"]) == -1 and b"overlap" in sim.h.L.avsim_last_error(sim.h.h)
    # fmt 2, on either side
    L, c = sim.h.L, base.copy()
    p = np.array([(0, 0, 0, 0, 7, 5)], np.int32)
    for sf, df in ((2, 0), (0, 2)):
        assert L.avsim_compose(sim.h.h, src.ctypes.data, sf, 2, 34, 34, c.ctypes.data, df, 1, 20, 20, p.ctypes.data, 1, 1, 0) == -1
    assert L.avsim_compose(sim.h.h, src.ctypes.data, 0, 2, 34, 65536, c.ctypes.data, 0, 1, 20, 20, p.ctypes.data, 1, 1, 0) == -1
    assert np.array_equal(c, base)
    with pytest.raises(ValueError):
        sim.compose(src, bad["overlap"], canvas_hw=(20, 20))
    # the same places one image apart do not overlap; and the facade returns the reference's canvas
    ok = [(0, 0, 0, 0, 7, 5), (1, 1, 6, 4, 7, 5)]
    got = sim.compose(src, ok, canvas_hw=(20, 20), clear=0x010203)
    want = np.empty((2, 20, 20, 3), np.uint8)
    want[:] = (1, 2, 3)
    assert np.array_equal(got, compose.compose_reference(want, src, ok))


def test_labels_equal_the_reference(sim, dev):
    h, d = dev
    values = [0, 7, 1234567890123, -45, -(1 << 63)]
    CH, CW = 30, 150
    base = noise((len(values), CH, CW, 3), 5)
    where = [(i, 3 + i, 2, 1 + (i == 1)) for i in range(len(values))]
    want = compose.label_reference(base.copy(), where, "EP ", values, 0xFFEE01)
    assert not np.array_equal(want, base)
    wa = np.ascontiguousarray(where, dtype=np.int32)
    # host pointers, u8 canvas, through the facade
    assert np.array_equal(sim.compose_label(base.copy(), where, "EP ", values, 0xFFEE01), want)
    # device pointers: the values live in a device tensor; both canvas formats, with guard bytes around the canvas
    tv = T.tensor(values, dtype=T.int64, device=d)
    for df in (0, 1):
        nbytes = base.size * (4 if df else 1)
        whole, flat = guarded(nbytes)
        canvas = flat.view(T.float32).view(len(values), 3, CH, CW) if df else flat.view(len(values), CH, CW, 3)
        canvas.copy_(T.from_numpy(to_f32(base) if df else base).to(d))
        assert h.L.avsim_compose_label(h.h, canvas.data_ptr(), df, len(values), CH, CW, wa.ctypes.data, len(wa), b"EP ", tv.data_ptr(), 0xFFEE01) == 0
        T.cuda.synchronize()
        if df:
            assert T.equal(canvas.cpu(), T.from_numpy(to_f32(want)))
        else:
            assert np.array_equal(canvas.cpu().numpy(), want)
        assert guards_intact(whole, nbytes)
    # value NULL: the prefix alone; an unknown character draws nothing
    want = compose.label_reference(base.copy(), where, "RUN: a?9/=-.", None, 0x00FF00)
    tc = T.from_numpy(base.copy()).to(d)
    assert h.L.avsim_compose_label(h.h, tc.data_ptr(), 0, len(values), CH, CW, wa.ctypes.data, len(wa), b"RUN: a?9/=-.", None, 0x00FF00) == 0
    T.cuda.synchronize()
    assert np.array_equal(tc.cpu().numpy(), want)
    # labels that leave the canvas on every side are clipped, not refused, and write nothing outside it
    where = [(0, CW - 20, CH - 10, 3), (1, -7, -5, 2), (2, CW, 0, 1), (3, 0, CH + 5, 1), (4, -4000, -4000, 64)]
    wa = np.ascontiguousarray(where, dtype=np.int32)
    want = compose.label_reference(base.copy(), where, "ID ", values, 0xFFFFFF)
    whole, flat = guarded(base.size)
    canvas = flat.view(len(values), CH, CW, 3)
    canvas.copy_(T.from_numpy(base).to(d))
    assert h.L.avsim_compose_label(h.h, canvas.data_ptr(), 0, len(values), CH, CW, wa.ctypes.data, len(wa), b"ID ", tv.data_ptr(), 0xFFFFFF) == 0
    T.cuda.synchronize()
    assert np.array_equal(canvas.cpu().numpy(), want)
    assert guards_intact(whole, base.size)
    # refused: a scale of 0 or 65, an image index of nout, a prefix of 16 characters
    c = base.copy()
    for w4, prefix in (((0, 0, 0, 0), b"A"), ((0, 0, 0, 65), b"A"), ((len(values), 0, 0, 1), b"A"), ((0, 0, 0, 1), b"0123456789ABCDEF")):
        w1 = np.array([w4], np.int32)
        assert sim.h.L.avsim_compose_label(sim.h.h, c.ctypes.data, 0, len(values), CH, CW, w1.ctypes.data, 1, prefix, None, 0) == -1, (w4, prefix)
    assert np.array_equal(c, base)


def test_vec_env_compose():
    env = make_vec(PEG, num_envs=2, max_episode_steps=10, cameras=["zed_cam_left"], observation_height=48, observation_width=64)
    try:
        obs, info = env.reset(seed=3)
        img = obs["observation.images.zed_cam_left"]
        assert tuple(img.shape) == (2, 3, 48, 64)
        places = [(0, 0, 0, 0, 32, 24), (0, 1, 32, 0, 32, 24)]
        out = env.compose(img, places, canvas_hw=(24, 64))
        again = env.compose(img, places, canvas_hw=(24, 64))           # the same sizes and places: nothing is validated, uploaded or waited for
        env.compose_label(again, [(0, 1, 1, 1), (0, 33, 1, 1)], "", info["episode_id"], 0xFFFFFF)
        f = img.cpu().numpy()
        u8 = np.ascontiguousarray(((f * np.float32(255)) + np.float32(0.5)).astype(np.uint8).transpose(0, 2, 3, 1))      # the encoder's conversion
        assert len(np.unique(u8[0].reshape(-1, 3), axis=0)) > 20                                                         # a picture, not a flat field
        want = compose.compose_reference(np.zeros((1, 24, 64, 3), np.uint8), u8, places)
        assert np.array_equal(out.cpu().numpy(), want)
        compose.label_reference(want, [(0, 1, 1, 1), (0, 33, 1, 1)], "", info["episode_id"].cpu().numpy(), 0xFFFFFF)
        assert np.array_equal(again.cpu().numpy(), want)
        planes = env.compose(img, places, canvas_hw=(24, 64), fmt="lerobot")
        assert T.equal(planes.cpu(), T.from_numpy(to_f32(compose.compose_reference(np.zeros((1, 24, 64, 3), np.uint8), u8, places))))
        with pytest.raises(ValueError):
            env.compose(img, [(0, 2, 0, 0, 32, 24)], canvas_hw=(24, 64))
    finally:
        env.close()


DEVICE_IMAGES_ALONE = r"""
import numpy as np
import torch
from av_aloha_amd import compose, imgaug, imgprep, jpeg
from av_aloha_amd.images import DeviceImages
from av_aloha_amd.vec_env import make_vec

H, W, Q = 37, 53, 90
yy, xx = np.mgrid[0:H, 0:W]
u8 = np.stack([np.stack([(4 * xx + 40 * i) % 256, (5 * yy + 9 * i) % 256, (xx + yy + 30 * i) % 256], -1) for i in range(2)]).astype(np.uint8)
u8 ^= np.random.default_rng(0).integers(0, 8, u8.shape, dtype=np.uint8)
places = [(0, 0, 3, 1, W, H), (0, 1, 60, 2, 40, 30)]                   # a copy and a shrink, side by side on a 40 x 120 canvas
where, values, rgb = [(0, 5, 30, 1), (0, 62, 3, 2)], np.array([7, 123456], np.int64), 0x40FF80
box, mean, std = [(3, 2, 0), (13, 13, 1)], [0.4, 0.5, 0.6], [0.2, 0.25, 0.3]      # the second box flipped, flush with the corner
lut = np.ascontiguousarray(imgprep.normalise_lut(mean, std), dtype=np.float32)
params = (np.array([b[:2] + (b[2], 31) for b in box], np.int32), np.array([[1.2, 0.7, 1.4, 0.1, 1.8], [0.6, 1.5, 0.3, -0.2, 0.4]], np.float32))

# the numpy specifications, once
streams = [jpeg.encode_reference(f, Q) for f in u8]
dec = np.stack([jpeg.decode_reference(x) for x in streams])
want = {"gym": dec, "lerobot": dec.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255),
        "canvas": compose.compose_reference(np.zeros((1, 40, 120, 3), np.uint8), dec, places)}
want["label"] = compose.label_reference(want["canvas"].copy(), where, "E", values, rgb)
want["stats"] = imgprep.stats_reference(want["label"])
want["prep"] = imgprep.prep_reference(dec, lut, None, box, (24, 40))
want["jitter"] = imgaug.jitter_reference(dec, params, (24, 40), mean=mean, std=std)

ops = DeviceImages()                                                     # no env, no other handle: it brings torch's GPU up itself
dev = ops.device
t_u8, t_values, t_lut = (torch.from_numpy(a).to(dev) for a in (u8, values, lut))


def chain():
    out, ln = ops.encode_images(t_u8, Q)
    got = {"lerobot": ops.decode_jpeg(out, ln, height=H, width=W), "gym": ops.decode_jpeg(out, ln, height=H, width=W, fmt="gym")}
    img = got["gym"][0]
    got["canvas"] = ops.compose(img, places, canvas_hw=(40, 120)).clone()
    got["label"] = ops.compose_label(got["canvas"].clone(), where, "E", t_values, rgb)
    got["stats"] = ops.image_stats(got["label"])
    got["prep"] = ops.prep_images(img, t_lut, box, (24, 40))
    got["jitter"] = ops.jitter_images(img, params, (24, 40), mean=mean, std=std)
    n = ln.cpu().numpy()
    assert n.max() <= out.shape[1]
    assert [out[i, :n[i]].cpu().numpy().tobytes() for i in range(2)] == streams
    for k in ("lerobot", "gym"):
        assert not got[k][1].cpu().numpy().any()
        got[k] = got[k][0]
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == (np.int64 if k == "stats" else w.dtype) and g.shape == w.shape, k
        assert np.array_equal(g.view(w.dtype), w), k                      # (nothing here is a nan: bit for bit)


side = torch.cuda.Stream(device=dev)
side.wait_stream(torch.cuda.current_stream(dev))
with torch.cuda.stream(side):
    chain()
    assert ops._stream.cuda_stream == side.cuda_stream
side.synchronize()
chain()                                                                  # torch's current stream changed: the handle follows it
assert ops._stream.cuda_stream == torch.cuda.current_stream(dev).cuda_stream != side.cuda_stream
try:
    ops.decode_jpeg(*ops.encode_images(t_u8, Q))                          # no observation size to default to
    raise AssertionError("decode_jpeg without a size went through")
except ValueError:
    pass
ops.close()
ops.close()

env = make_vec("gym_guided_vision/InsertPeg-3Arms-v0", num_envs=2, max_episode_steps=5, cameras=[])
obs, info = env.reset(seed=1)
obs, reward, terminated, truncated, info = env.step(obs["observation.state"].clone())
assert info["elapsed_steps"].tolist() == [1, 1] and bool(torch.isfinite(obs["observation.state"]).all())
env.close()
print("device images alone: ok")
"""


def test_device_images_without_an_env():
    """images.DeviceImages in a process of its own, where no env and no other handle exists: the seven image calls on a side stream and then on
    torch's default stream, every result equal to its numpy specification bit for bit; close() twice; a VecEnv made afterwards steps."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.environ.get("PYTHONPATH", "")]))
    p = subprocess.run([sys.executable, "-c", DEVICE_IMAGES_ALONE], capture_output=True, text=True, env=env, cwd=root, timeout=300)
    assert p.returncode == 0 and "device images alone: ok" in p.stdout, p.stdout + p.stderr


def synthetic_episode(seed, T=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:36, 0:48]
    smooth = np.stack([np.stack([(4 * xx + 17 * t + 40 * seed) % 256, (5 * yy + 9 * t) % 256, (xx + yy + 30 * t) % 256], -1) for t in range(T)]).astype(np.uint8)
    return {"/observations/qpos": rng.standard_normal((T, 21)).astype(np.float32), "/observations/qvel": np.zeros((T, 21), np.float32),
            "/observations/all_qpos": np.zeros((T, 30), np.float32), "/action": np.zeros((T, 21), np.float32),
            "/observations/images/cam_a": rng.integers(0, 256, (T, 24, 32, 3), dtype=np.uint8), "/observations/images/cam_b": smooth}


def test_visualize_on_the_device_equals_the_host_path(tmp_path):
    data = synthetic_episode(0)
    files = {"raw": harness.save_episode(data, str(tmp_path / "raw"), 0, use_h5py=False),
             "packed": harness.save_episode(data, str(tmp_path / "packed"), 0, use_h5py=False, jpeg_quality=90)}
    for name, path in files.items():
        a, b = str(tmp_path / f"{name}_host.avi"), str(tmp_path / f"{name}_dev.avi")
        harness.visualize_episode(path, a, label="T=0", device="host")
        res = harness.visualize_episode(path, b, label="T=0", device=0, chunk_bytes=2 * (24 * 32 + 36 * 48 + 2 * 24 * 64) * 3)     # two frames a chunk
        assert res["frames"] == 3
        assert open(a, "rb").read() == open(b, "rb").read(), name                # the AVI payload included
        if name == "packed":                                                      # only streams crossed the bus, in either direction
            assert res["bytes_to_device"] < 3 * (24 * 32 + 36 * 48) * 3 * 2 and res["bytes_from_device"] < 3 * 24 * 64 * 3 * 2
    # the data set's video: two files, every second frame, numbered labels
    d = str(tmp_path / "set")
    for i in range(2):
        harness.save_episode(synthetic_episode(i + 1), d, i, use_h5py=False, jpeg_quality=90)
    a, b = str(tmp_path / "set_host.avi"), str(tmp_path / "set_dev.avi")
    harness.visualize_dataset(os.path.join(d, "episode_*.hdf5"), a, stride=2, label="E", device="host")
    harness.visualize_dataset(os.path.join(d, "episode_*.hdf5"), b, stride=2, label="E", device=0)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert mjpeg.read_avi(b)[0]["frames"] == 4


def test_evaluate_vec_grid_video(tmp_path):
    env = make_vec(PEG, num_envs=4, max_episode_steps=3, cameras=["zed_cam_left"], observation_height=48, observation_width=64)
    try:
        ids = []

        def policy(obs, info):
            ids.append(info["episode_id"].cpu().numpy().copy())
            return T.zeros((4, env.nj), dtype=T.float32, device=env.device)
        plain = harness.evaluate_vec(env, policy, 6, seed=5)
        calls_plain, ids[:] = len(ids), []
        path = str(tmp_path / "grid" / "batch.avi")
        with_grid = harness.evaluate_vec(env, policy, 6, seed=5, grid_video=path, grid_envs=4, grid_cell=(24, 32))
        calls = len(ids)
        assert calls == calls_plain
        assert len(plain) == len(with_grid) == 6
        for a, b in zip(plain, with_grid):                                        # the records do not depend on the grid
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        info, frames = mjpeg.read_avi(path)
        assert (info["frames"], info["height"], info["width"]) == (calls, 48, 64)          # a frame per step call, 2 x 2 cells of 24 x 32
        pics = [jpeg.decode_reference(f).astype(int) for f in frames]
        # frame j shows the ids the policy saw in call j + 1; where an env's id changes from one frame to the next, its cell's label changes
        rows, _, _ = compose.layout_grid(4, 24, 32)
        changes = 0
        for j in range(1, calls - 1):
            for e, (x0, y0, w, h) in enumerate(rows):
                if ids[j + 1][e] != ids[j][e]:
                    region = (slice(y0 + 2, y0 + 10), slice(x0 + 2, x0 + 14))
                    assert (pics[j][region] != pics[j - 1][region]).any(), (j, e)
                    changes += 1
        assert changes >= 4                                                       # every env went on to a second episode
        with pytest.raises(ValueError):
            harness.evaluate_vec(env, policy, 1, grid_video=path, grid_envs=5)
        with pytest.raises(ValueError):
            harness.evaluate_vec(env, policy, 1, grid_video=path, grid_envs=2, video_camera="overhead_cam")
    finally:
        env.close()
