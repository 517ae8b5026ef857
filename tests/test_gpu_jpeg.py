"""The device JPEG encoder (avsim_jpeg_encode, csrc/avsim_jpeg.hip.h) against its specification, av_aloha_amd/jpeg.py encode_reference:
equal byte for byte, lengths included -- every step is integer arithmetic, so there is no tolerance.  Then the layers above it:
BatchedSim.encode_jpeg, VecEnv.encode_jpeg, the videos of harness.evaluate_vec and harness.rollout.  (No decoder here: that the stream is
a JPEG every decoder reads is tests/test_jpeg_host.py's subject.)"""
import os

import numpy as np
import pytest

from av_aloha_amd import _ffi, jpeg
from av_aloha_amd.mjpeg import read_avi
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import make_vec, sample_poses
from gpu_util import device_handle, torch as T
from gpu_util import sim          # noqa: F401  (a module-scoped fixture: this module gets its own handle)

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"


def images():
    rng = np.random.default_rng(0)
    g = np.linspace(0, 255, 160).astype(np.uint8)
    return {"noise_37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
            "noise_96x128": rng.integers(0, 256, (96, 128, 3), dtype=np.uint8),
            "noise_20x330": rng.integers(0, 256, (20, 330, 3), dtype=np.uint8),      # 21 MCUs per row: chunks of 10, 10 and 1
            "white_32x48": np.full((32, 48, 3), 255, np.uint8),
            "ramp_120x160": np.stack([np.tile(g, (120, 1)), np.tile(g[::-1], (120, 1)), np.full((120, 160), 77, np.uint8)], -1)}


def encode_host(sim, imgs, quality, fmt=0, index=None, stride=None):
    """avsim_jpeg_encode through a host-pointer handle -> (streams, out_len)."""
    imgs = np.ascontiguousarray(imgs)
    H, W = (imgs.shape[1], imgs.shape[2]) if fmt == 0 else (imgs.shape[2], imgs.shape[3])
    n = len(imgs) if index is None else len(index)
    stride = int(sim.h.L.avsim_jpeg_bound(H, W)) if stride is None else stride
    out, ln = np.zeros((n, stride), np.uint8), np.zeros(n, np.int32)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    sim.h.check(sim.h.L.avsim_jpeg_encode(sim.h.h, imgs.ctypes.data, fmt, _ffi.ptr(idx), n, H, W, quality, out.ctypes.data, stride, ln.ctypes.data))
    return [out[i, :ln[i]].tobytes() for i in range(n)], ln


def test_bound_and_argument_errors(sim):
    L = sim.h.L
    for H, W in ((480, 640), (37, 53), (1, 1), (65535, 16)):
        assert L.avsim_jpeg_bound(H, W) == jpeg.bound(H, W)
    assert L.avsim_jpeg_bound(0, 5) == _ffi.lib().avsim_jpeg_bound(5, 65536) == -1
    img, out, ln = np.zeros((1, 16, 16, 3), np.uint8), np.zeros((1, 4096), np.uint8), np.zeros(1, np.int32)
    for fmt, H, W, q in ((2, 16, 16, 90), (0, 16, 16, 0), (0, 16, 16, 101), (0, 0, 16, 90), (0, 16, 65536, 90)):
        assert L.avsim_jpeg_encode(sim.h.h, img.ctypes.data, fmt, None, 1, H, W, q, out.ctypes.data, 4096, ln.ctypes.data) == -1, (fmt, H, W, q)


@pytest.mark.parametrize("quality", [50, 90, 100])
def test_synthetic_images_equal_the_reference(sim, quality):
    for name, img in images().items():
        want = jpeg.encode_reference(img, quality)
        got, ln = encode_host(sim, img[None], quality)
        assert ln[0] == len(want), (name, quality, int(ln[0]), len(want))
        assert got[0] == want, (name, quality, next(i for i in range(len(want)) if got[0][i] != want[i]))
        assert sim.encode_jpeg(img, quality) == [want], (name, quality)
        if name.startswith("noise") and quality == 100:
            assert len(want) <= sim.h.L.avsim_jpeg_bound(*img.shape[:2])


@pytest.mark.parametrize("task", ["insert_peg", "tube_transfer"])
def test_rendered_frames_equal_the_reference_in_both_formats(task):
    s = BatchedSim(task, 3, 2, options={"render_shadows": 1, "render_samples": 4, "render_smooth": 1})
    s.reset(sample_poses(task, 1, [0, 1]))
    cams = ["zed_cam_left", "wrist_cam_right"]
    ids = np.array([s.manifest["camera_names"].index(c) for c in cams], dtype=np.int32)
    for H, W in ((480, 640), (120, 160)):
        u8 = s.render_rgb(cams, H, W)                              # [2, 2, H, W, 3]
        f32 = np.zeros((2, 2, 3, H, W), np.float32)
        s.h.check(s.h.L.avsim_render_rgb_f32(s.h.h, ids.ctypes.data, 2, H, W, f32.ctypes.data))
        assert np.array_equal((f32 * 255 + 0.5).astype(np.uint8), u8.transpose(0, 1, 4, 2, 3))
        assert len(np.unique(u8[0, 0].reshape(-1, 3), axis=0)) > 100        # a picture, not a flat field
        for q in (50, 90, 100):
            a, la = encode_host(s, u8.reshape(4, H, W, 3), q)
            b, lb = encode_host(s, f32.reshape(4, 3, H, W), q, fmt=1)
            assert a == b and np.array_equal(la, lb), (task, H, q)
            for i in range(4):                                     # (two envs x two cameras)
                want = jpeg.encode_reference(u8.reshape(4, H, W, 3)[i], q)
                assert la[i] == len(want) and a[i] == want, (task, H, q, i)
    s.close()


def test_batch_with_an_index_on_host_and_device_handles(sim):
    rng = np.random.default_rng(7)
    imgs = rng.integers(0, 256, (64, 48, 80, 3), dtype=np.uint8)
    imgs[::3] //= 4                                                  # some darker, shorter streams in between
    imgs[5] = 255
    index = rng.permutation(64).astype(np.int32)
    index[10:20] = index[0]                                          # repeats
    index[63] = 63
    want = [jpeg.encode_reference(imgs[i], 90) for i in range(64)]
    got, ln = encode_host(sim, imgs, 90, index=index)
    assert got == [want[i] for i in index]
    # device pointers: nothing but the handle's I/O mode differs
    h, dev = device_handle()
    stride = 16384
    d_img, d_idx = T.from_numpy(imgs).to(dev), T.from_numpy(index).to(dev)
    out, dl = T.zeros((64, stride), dtype=T.uint8, device=dev), T.zeros(64, dtype=T.int32, device=dev)
    h.check(h.L.avsim_jpeg_encode(h.h, d_img.data_ptr(), 0, d_idx.data_ptr(), 64, 48, 80, 90, out.data_ptr(), stride, dl.data_ptr()))
    o, l = out.cpu().numpy(), dl.cpu().numpy()
    assert [o[i, :l[i]].tobytes() for i in range(64)] == [want[i] for i in index]
    # the float planes of the same images, without an index
    d_f32 = (d_img.permute(0, 3, 1, 2).contiguous().to(T.float32) / 255)
    h.check(h.L.avsim_jpeg_encode(h.h, d_f32.data_ptr(), 1, None, 64, 48, 80, 90, out.data_ptr(), stride, dl.data_ptr()))
    o, l = out.cpu().numpy(), dl.cpu().numpy()
    assert [o[i, :l[i]].tobytes() for i in range(64)] == want
    h.close()


def test_a_stream_longer_than_the_stride_is_cut_at_the_stride():
    rng = np.random.default_rng(2)
    imgs = np.full((3, 64, 64, 3), 255, np.uint8)
    imgs[1] = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    want = [jpeg.encode_reference(im, 100) for im in imgs]
    stride = len(want[0]) + 101
    assert len(want[1]) > 3 * stride                                 # the noise image would run over both neighbours and the tail
    h, dev = device_handle()
    buf = T.full((3 * stride + len(want[1]) + 4096,), 0xAA, dtype=T.uint8, device=dev)
    dl = T.zeros(3, dtype=T.int32, device=dev)
    h.check(h.L.avsim_jpeg_encode(h.h, T.from_numpy(imgs).to(dev).data_ptr(), 0, None, 3, 64, 64, 100, buf.data_ptr(), stride, dl.data_ptr()))
    o, l = buf.cpu().numpy(), dl.cpu().numpy()
    assert l.tolist() == [len(w) for w in want]
    assert (o[3 * stride:] == 0xAA).all()                            # nothing past the three slots
    for i in (0, 2):
        assert o[i * stride:i * stride + l[i]].tobytes() == want[i]
        assert (o[i * stride + l[i]:(i + 1) * stride] == 0xAA).all()
    h.close()


def _policy_for(env):
    base = []

    def policy(obs, info):
        if not base:
            base.append(env._ap.float().clone())                     # the reset pose: the same in every env
        a = base[0].clone()
        a[:, :6] += 0.05 * T.sin(0.5 * info["elapsed_steps"].to(T.float32) + info["episode_id"].to(T.float32))[:, None]
        return a
    return policy


def test_evaluate_vec_writes_the_first_episodes_videos(tmp_path):
    from av_aloha_amd.harness import evaluate_vec
    kw = dict(cameras=["zed_cam_left"], seed=3, observation_height=120, observation_width=160)
    env = make_vec(PEG, 8, 12, obs_format="lerobot", **kw)
    recs = evaluate_vec(env, _policy_for(env), 8, video_dir=str(tmp_path / "v"), video_episodes=4, video_quality=90, video_fps=25)
    env.close()
    env = make_vec(PEG, 8, 12, obs_format="lerobot", **kw)
    plain = evaluate_vec(env, _policy_for(env), 8)
    env.close()
    assert len(recs) == len(plain) == 8
    for a, b in zip(recs, plain):
        assert {k: v for k, v in a.items() if k != "initial_object_poses"} == {k: v for k, v in b.items() if k != "initial_object_poses"}
        assert np.array_equal(a["initial_object_poses"], b["initial_object_poses"])
    assert sorted(os.listdir(str(tmp_path / "v"))) == [f"rollout_{i}.avi" for i in range(4)]
    # the u8 frames of the same episodes from a gym-format env, and its own encoder calls
    env = make_vec(PEG, 8, 12, obs_format="gym", **kw)
    policy = _policy_for(env)
    env.start_log(8)
    obs, info = env.reset()
    frames = []
    for t in range(12):
        obs, _, _, _, info = env.step(policy(obs, info))
        frames.append(obs["pixels"]["zed_cam_left"][:4].cpu().numpy().copy())
        if t == 5:
            idx = T.tensor([3, 1, 1, 7], dtype=T.int32, device=env.device)
            o, l = env.encode_jpeg("zed_cam_left", envs=idx, quality=75)
            full = obs["pixels"]["zed_cam_left"].cpu().numpy()
            o, l = o.cpu().numpy(), l.cpu().numpy()
            assert [o[i, :l[i]].tobytes() for i in range(4)] == [jpeg.encode_reference(full[e], 75) for e in (3, 1, 1, 7)]
            o, l = env.encode_jpeg("zed_cam_left", envs=2)
            assert tuple(o.shape) == (2, env.jpeg_stride()) and o[1, :int(l[1])].cpu().numpy().tobytes() == jpeg.encode_reference(full[1], 90)
    with pytest.raises(ValueError):
        env.encode_jpeg("overhead_cam")
    env.close()
    for e in range(4):
        info_e, got = read_avi(str(tmp_path / "v" / f"rollout_{e}.avi"))
        assert info_e == {"frames": recs[e]["length"], "width": 160, "height": 120, "fps": 25.0, "codec": "MJPG"} and recs[e]["length"] == 12
        for t in range(12):
            assert got[t] == jpeg.encode_reference(frames[t][e], 90), (e, t)
    assert any(len(set(f[e].tobytes() for f in frames)) > 1 for e in range(4))       # the arm moves: the frames differ


def test_rollout_writes_an_avi(tmp_path):
    from av_aloha_amd.env import make
    from av_aloha_amd.harness import rollout
    env = make(PEG, cameras=["zed_cam_left"], observation_height=120, observation_width=160)
    res = rollout(env, lambda obs: obs["observation.state"].numpy(), 3, num_episodes=2, video_path=str(tmp_path / "out" / "rollout_{}.avi"))
    env.close()
    for i in range(2):
        info, got = read_avi(str(tmp_path / "out" / f"rollout_{i}.avi"))
        assert info["frames"] == 3 and (info["width"], info["height"], info["fps"]) == (160, 120, 50.0)
        assert got == [jpeg.encode_reference(f, 90) for f in res[i]["frames"]]
