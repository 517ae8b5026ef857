"""avsim_render_jpeg: frames rendered and encoded without leaving the device give the streams of avsim_jpeg_encode on avsim_render_rgb's
frames, byte for byte -- per view, and with an env's views side by side (the Cartesian env's zed_cam) --, through host and device
handles; the recorder's image_streams are those bytes.  And avsim_jpeg_decode when its staging budget makes it walk a batch in groups."""
import os

import numpy as np
import pytest

from av_aloha_amd import jpeg
from av_aloha_amd.constants import MODEL_DIR
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import sample_poses
from gpu_util import device_handle, torch as T

pytestmark = pytest.mark.gpu

OPTIONS = {"render_shadows": 1, "render_samples": 4, "render_smooth": 1}
CAMS = ["zed_cam_left", "zed_cam_right"]


@pytest.fixture(scope="module")
def sim():
    s = BatchedSim("insert_peg", 3, 3, options=OPTIONS)
    s.reset(sample_poses("insert_peg", 1, [0, 1, 2]))
    yield s
    s.close()


# 160: rows of whole dwords; 53: rows of 159 bytes, the tile kernel's byte path, and partial MCUs
@pytest.mark.parametrize("H,W", [(120, 160), (37, 53)])
def test_streams_equal_those_of_the_rendered_frames(sim, H, W):
    u8 = sim.render_rgb(CAMS, H, W)                                      # [3, 2, H, W, 3]
    assert len(np.unique(u8[0, 0].reshape(-1, 3), axis=0)) > 50           # a picture, not a flat field
    per_view = sim.render_jpeg(CAMS, H, W, 90)
    assert [len(v) for v in per_view] == [2, 2, 2]
    want = sim.encode_jpeg(u8.reshape(6, H, W, 3), 90)
    assert [s for v in per_view for s in v] == want
    assert want[0] == jpeg.encode_reference(u8[0, 0], 90)
    tiled = sim.render_jpeg(CAMS, H, W, 75, tile=True)
    side = np.concatenate([u8[:, 0], u8[:, 1]], axis=2)                   # [3, H, 2 W, 3], as sim_env puts zed_cam together
    assert tiled == sim.encode_jpeg(side, 75)
    assert jpeg.stream_size(tiled[0]) == (H, 2 * W)


def test_small_tiled_streams_equal_those_of_the_tiled_frames(sim):
    """8 x 12 views side by side: the rendered and the tiled images are scratch of the call, far smaller than the 120 x 160 ones the same buffers served."""
    H, W = 8, 12
    u8 = sim.render_rgb(CAMS, H, W)
    tiled = sim.render_jpeg(CAMS, H, W, 90, tile=True)
    assert tiled == sim.encode_jpeg(np.concatenate([u8[:, 0], u8[:, 1]], axis=2), 90)
    assert len(tiled) == 3 and jpeg.stream_size(tiled[0]) == (H, 2 * W)


def test_a_short_stride_reports_the_length_and_keeps_to_its_rows(sim):
    H, W = 120, 160
    full = [s for v in sim.render_jpeg(CAMS, H, W, 90) for s in v]
    ids = np.array([sim.manifest["camera_names"].index(c) for c in CAMS], dtype=np.int32)
    stride = min(len(s) for s in full) - 7
    buf, ln = np.full((6 + 1, stride), 0xAA, np.uint8), np.zeros(6, np.int32)
    sim.h.check(sim.h.L.avsim_render_jpeg(sim.h.h, ids.ctypes.data, 2, H, W, 0, 90, buf.ctypes.data, stride, ln.ctypes.data))
    assert ln.tolist() == [len(s) for s in full]
    assert all(buf[i].tobytes() == full[i][:stride] for i in range(6)) and (buf[6] == 0xAA).all()
    for args in ((2, H, W, 0, 0), (2, H, W, 0, 101), (2, 0, W, 0, 90), (2, H, 40000, 1, 90), (0, H, W, 0, 90)):
        ncam, h_, w_, tile, q = args
        assert sim.h.L.avsim_render_jpeg(sim.h.h, ids.ctypes.data, ncam, h_, w_, tile, q, buf.ctypes.data, stride, ln.ctypes.data) == -1, args


def test_device_handle_writes_the_same_streams():
    H, W = 120, 160
    poses = sample_poses("insert_peg", 1, [0, 1])
    host = BatchedSim("insert_peg", 3, 2, options=OPTIONS)
    host.reset(poses)
    want = host.render_jpeg(CAMS, H, W, 90, tile=True)
    host.close()
    h, dev = device_handle()
    L = h.L
    for k, v in OPTIONS.items():
        h.check(L.avsim_set_option(h.h, k.encode(), float(v)))
    with open(os.path.join(MODEL_DIR, "visual_meshes.avv"), "rb") as f:
        lib = f.read()
    h.check(L.avsim_load_visual(h.h, lib, len(lib)))
    h.check(L.avsim_reset(h.h, None, T.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).to(dev).data_ptr()))
    ids = np.array([host.manifest["camera_names"].index(c) for c in CAMS], dtype=np.int32)
    stride = max(len(s) for s in want) + 64
    buf, ln = T.full((2, stride), 0xAA, dtype=T.uint8, device=dev), T.zeros(2, dtype=T.int32, device=dev)
    h.check(L.avsim_render_jpeg(h.h, ids.ctypes.data, 2, H, W, 1, 90, buf.data_ptr(), stride, ln.data_ptr()))
    b, l = buf.cpu().numpy(), ln.cpu().numpy()
    assert [b[i, :l[i]].tobytes() for i in range(2)] == want
    assert all((b[i, l[i]:] == 0xAA).all() for i in range(2))
    h.close()


def test_cartesian_env_image_streams_are_its_images_encoded():
    from av_aloha_amd.sim_env import make_sim_env
    env = make_sim_env("sim_insert_peg", cameras=["zed_cam", "cam_right_wrist"], num_envs=2)
    env.sim.reset(sample_poses("insert_peg", 1, [0, 1]))
    obs = env.get_obs()
    streams = env.image_streams(90)
    assert "images" not in env.get_obs(images=False) and sorted(streams) == ["cam_right_wrist", "zed_cam"]
    for cam, (H, W) in (("zed_cam", (720, 1440)), ("cam_right_wrist", (480, 640))):
        assert obs["images"][cam].shape == (2, H, W, 3)
        assert streams[cam] == env.sim.encode_jpeg(obs["images"][cam], 90), cam
    env.close()


def test_decode_in_groups_of_images():
    """A staging budget below the batch's coefficients: the decoder goes through the batch in groups (here of 2, 2 and 1 images)."""
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (5, 37, 53, 3), dtype=np.uint8)
    streams = [jpeg.encode_reference(im, (50, 90, 100)[i % 3]) for i, im in enumerate(imgs)]
    s = BatchedSim("insert_peg", 3, 2)
    per_img = 3 * 4 * 384 * 2                                            # int16 coefficients of the 3 x 4 MCUs of a 37 x 53 image
    s.set_option("jpeg_decode_budget", 2 * per_img + 100)
    for mode in ("replicate", "triangle"):
        got = s.decode_jpeg(streams, upsample=mode)
        for i in range(5):
            assert np.array_equal(got[i], jpeg.decode_reference(streams[i], mode)), (mode, i)
    bad = list(streams)
    bad[4] = bad[4][:-2] + b"\x00\x00"                                   # the last group's image without its EOI: its own status, not a neighbour's
    with pytest.raises(jpeg.JpegError) as e:
        s.decode_jpeg(bad)
    assert e.value.status == jpeg.STATUS_STRUCTURE and "stream 4" in str(e.value)
    s.close()
