"""The device JPEG decoder (avsim_jpeg_decode, csrc/avsim_jpeg.hip.h) against its specification, av_aloha_amd/jpeg.py decode_reference:
equal byte for byte in both upsampling modes and both output formats -- every step is integer arithmetic, so there is no tolerance.  Then
the status bits of streams that are not this encoder's, and the layers above the C call: BatchedSim.decode_jpeg, VecEnv.decode_jpeg, the
compressed episode files of harness.record_scripted and dataset.CompressedDataset.  (That decode_reference shows what an independent
decoder shows is tests/test_jpeg_decode_host.py's subject.)"""
import io
import os

import numpy as np
import pytest

from av_aloha_amd import _ffi, jpeg
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import make_vec, sample_poses
from gpu_util import device_handle, torch as T
from gpu_util import sim          # noqa: F401  (a module-scoped fixture: this module gets its own handle)

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
MODES = ("replicate", "triangle")
GUARD = 4096


def images():
    """The encoder tests' five images and three small ones: a single pixel, one whole MCU, one pixel more than an MCU in both directions."""
    rng = np.random.default_rng(0)
    g = np.linspace(0, 255, 160).astype(np.uint8)
    return {"noise_37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),      # partial MCUs on both edges
            "noise_96x128": rng.integers(0, 256, (96, 128, 3), dtype=np.uint8),
            "noise_20x330": rng.integers(0, 256, (20, 330, 3), dtype=np.uint8),    # 21 MCUs per row: three workgroups of the reconstruction
            "white_32x48": np.full((32, 48, 3), 255, np.uint8),
            "ramp_120x160": np.stack([np.tile(g, (120, 1)), np.tile(g[::-1], (120, 1)), np.full((120, 160), 77, np.uint8)], -1),
            "noise_1x1": rng.integers(0, 256, (1, 1, 3), dtype=np.uint8),
            "noise_16x16": rng.integers(0, 256, (16, 16, 3), dtype=np.uint8),
            "noise_17x33": rng.integers(0, 256, (17, 33, 3), dtype=np.uint8)}


def pack(streams, stride=None):
    stride = max(len(s) for s in streams) if stride is None else stride
    buf, ln = np.zeros((len(streams), stride), np.uint8), np.array([len(s) for s in streams], np.int32)
    for i, s in enumerate(streams):
        buf[i, :len(s)] = np.frombuffer(s, np.uint8)
    return buf, ln


def decode_host(sim, streams, H, W, fmt=0, upsample="replicate", index=None):
    """avsim_jpeg_decode through a host-pointer handle -> (images, status)."""
    buf, ln = pack(streams)
    n = len(streams) if index is None else len(index)
    out = np.zeros((n, H, W, 3), np.uint8) if fmt == 0 else np.zeros((n, 3, H, W), np.float32)
    status = np.full(n, -1, np.int32)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    sim.h.check(sim.h.L.avsim_jpeg_decode(sim.h.h, buf.ctypes.data, buf.shape[1], ln.ctypes.data, _ffi.ptr(idx), n, H, W, fmt, MODES.index(upsample),
                                          out.ctypes.data, status.ctypes.data))
    return out, status


def host_status(stream):
    """What the specification says of a stream: 0, or the status bit of the error it raises."""
    try:
        jpeg.decode_reference(stream)
        return 0
    except jpeg.JpegError as e:
        return e.status


def test_argument_errors(sim):
    L = sim.h.L
    s = jpeg.encode_reference(np.zeros((16, 16, 3), np.uint8), 90)
    buf, ln = pack([s])
    out, st = np.zeros((1, 16, 16, 3), np.uint8), np.zeros(1, np.int32)
    for stride, H, W, fmt, up in ((len(s), 16, 16, 2, 0), (len(s), 16, 16, 0, 2), (len(s), 0, 16, 0, 0), (len(s), 16, 65536, 0, 0), (0, 16, 16, 0, 0)):
        assert L.avsim_jpeg_decode(sim.h.h, buf.ctypes.data, stride, ln.ctypes.data, None, 1, H, W, fmt, up, out.ctypes.data, st.ctypes.data) == -1, (stride, H, W, fmt, up)
    with pytest.raises(ValueError):
        sim.decode_jpeg([s], upsample="bilinear")


@pytest.mark.parametrize("quality", [50, 90, 100])
def test_synthetic_images_equal_the_reference(sim, quality):
    for name, img in images().items():
        H, W, _ = img.shape
        s = jpeg.encode_reference(img, quality)
        for mode in MODES:
            want = jpeg.decode_reference(s, mode)
            got, st = decode_host(sim, [s], H, W, 0, mode)
            assert st[0] == 0, (name, quality, mode, int(st[0]))
            assert np.array_equal(got[0], want), (name, quality, mode, int(np.abs(got[0].astype(int) - want).max()))
            f32, st = decode_host(sim, [s], H, W, 1, mode)
            assert st[0] == 0
            assert T.equal(T.from_numpy(f32[0]), T.from_numpy(want).permute(2, 0, 1).float() / 255), (name, quality, mode)
        assert np.array_equal(sim.decode_jpeg([s])[0], jpeg.decode_reference(s)), (name, quality)


@pytest.mark.parametrize("task", ["insert_peg", "tube_transfer"])
def test_rendered_frames_equal_the_reference(task):
    s = BatchedSim(task, 3, 2, options={"render_shadows": 1, "render_samples": 4, "render_smooth": 1})
    s.reset(sample_poses(task, 1, [0, 1]))
    u8 = s.render_rgb(["zed_cam_left", "wrist_cam_right"], 120, 160).reshape(4, 120, 160, 3)
    assert len(np.unique(u8[0].reshape(-1, 3), axis=0)) > 100            # a picture, not a flat field
    streams = s.encode_jpeg(u8, 90)
    for mode in MODES:
        got = s.decode_jpeg(streams, upsample=mode)
        for i in range(4):
            assert np.array_equal(got[i], jpeg.decode_reference(streams[i], mode)), (task, mode, i)
    if task == "insert_peg":                                             # one full-size frame
        big = s.render_rgb(["zed_cam_left"], 480, 640)[0, 0]
        stream = s.encode_jpeg(big, 90)[0]
        for mode in MODES:
            assert np.array_equal(s.decode_jpeg([stream], upsample=mode)[0], jpeg.decode_reference(stream, mode)), mode
    s.close()


def test_batch_of_mixed_qualities_with_an_index_on_host_and_device_handles(sim):
    rng = np.random.default_rng(7)
    imgs = rng.integers(0, 256, (12, 48, 80, 3), dtype=np.uint8)
    imgs[::3] //= 4                                                      # some darker, shorter streams in between
    imgs[5] = 255
    streams = [jpeg.encode_reference(imgs[i], (50, 90, 100)[i % 3]) for i in range(12)]
    want = {m: [jpeg.decode_reference(s, m) for s in streams] for m in MODES}
    index = rng.permutation(12).astype(np.int32)
    index[3:6] = index[0]                                                # repeats
    for mode in MODES:
        got, st = decode_host(sim, streams, 48, 80, 0, mode)
        assert not st.any() and all(np.array_equal(got[i], want[mode][i]) for i in range(12)), mode
        got, st = decode_host(sim, streams, 48, 80, 0, mode, index=index)
        assert not st.any() and all(np.array_equal(got[i], want[mode][j]) for i, j in enumerate(index)), mode
    # device pointers: nothing but the handle's I/O mode differs.  `out` is written by three calls in a row with nothing waiting in between
    h, dev = device_handle()
    buf, ln = pack(streams)
    d_buf, d_len, d_idx = T.from_numpy(buf).to(dev), T.from_numpy(ln).to(dev), T.from_numpy(index).to(dev)
    out, st = T.zeros((12, 48, 80, 3), dtype=T.uint8, device=dev), T.zeros(12, dtype=T.int32, device=dev)
    f32 = T.zeros((12, 3, 48, 80), dtype=T.float32, device=dev)
    args = (d_buf.data_ptr(), buf.shape[1], d_len.data_ptr())
    h.check(h.L.avsim_jpeg_decode(h.h, *args, None, 12, 48, 80, 0, 1, out.data_ptr(), st.data_ptr()))
    first = out.clone()
    h.check(h.L.avsim_jpeg_decode(h.h, *args, d_idx.data_ptr(), 12, 48, 80, 0, 0, out.data_ptr(), st.data_ptr()))
    second = out.clone()
    h.check(h.L.avsim_jpeg_decode(h.h, *args, None, 12, 48, 80, 0, 0, out.data_ptr(), st.data_ptr()))
    h.check(h.L.avsim_jpeg_decode(h.h, *args, None, 12, 48, 80, 1, 0, f32.data_ptr(), st.data_ptr()))
    assert not st.cpu().numpy().any()
    assert np.array_equal(first.cpu().numpy(), np.stack(want["triangle"]))
    assert np.array_equal(second.cpu().numpy(), np.stack([want["replicate"][j] for j in index]))
    assert np.array_equal(out.cpu().numpy(), np.stack(want["replicate"]))
    # (divided on the host: on the device torch multiplies by a rounded 1 / 255, which is not (float)u8 / 255 in every last bit)
    assert T.equal(f32.cpu(), out.cpu().permute(0, 3, 1, 2).float() / 255)
    h.close()


def corrupt_batch():
    """Six 37 x 53 streams, four of them spoilt on the host: (streams, lengths to pass, the specification's status of each)."""
    from PIL import Image
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (6, 37, 53, 3), dtype=np.uint8)
    streams = [jpeg.encode_reference(im, 90) for im in imgs]
    lengths = [len(s) for s in streams]
    lengths[1] //= 2                                                     # in_len cut to half
    bad = None                                                           # one entropy byte replaced so that the bounded decode of the specification objects
    for pos in range(jpeg.HEADER_BYTES + 40, len(streams[2]) - 2):
        s = bytearray(streams[2])
        if 0xFF in s[pos - 1:pos + 2] or s[pos] ^ 0x5A == 0xFF:
            continue
        s[pos] ^= 0x5A
        if host_status(bytes(s)) == jpeg.STATUS_ENTROPY:
            bad = bytes(s)
            break
    assert bad is not None
    streams[2] = bad
    b = io.BytesIO()
    Image.fromarray(imgs[3]).save(b, "JPEG", quality=90)                 # Pillow's own structure: no restart intervals, so another header
    streams[3], lengths[3] = b.getvalue(), len(b.getvalue())
    rst = streams[4].index(b"\xff\xd0", jpeg.HEADER_BYTES)
    streams[4] = streams[4][:rst] + streams[4][rst + 2:]                 # a missing RST
    lengths[4] -= 2
    want = [host_status(s[:n]) for s, n in zip(streams, lengths)]
    assert want == [0, jpeg.STATUS_STRUCTURE, jpeg.STATUS_ENTROPY, jpeg.STATUS_HEADER, jpeg.STATUS_STRUCTURE, 0]
    return streams, lengths, want


def test_corrupt_streams_get_their_status_and_nothing_else_is_touched():
    """Error reporting, not fault hunting: the kernels bound every read and write themselves (csrc/avsim_jpeg.hip.h).  The C call has no
    output stride, so the gaps between image slots are made by one call per image into slots GUARD bytes apart."""
    H, W = 37, 53
    streams, lengths, want = corrupt_batch()
    good = {i: jpeg.decode_reference(streams[i]) for i in (0, 5)}
    h, dev = device_handle()
    buf, _ = pack(streams)
    d_buf, d_len = T.from_numpy(buf).to(dev), T.tensor(lengths, dtype=T.int32, device=dev)
    for fmt, px in ((0, 1), (1, 4)):
        slot = H * W * 3 * px
        whole = T.full((GUARD + 6 * slot + GUARD,), 0xAA, dtype=T.uint8, device=dev)
        st = T.full((6,), -1, dtype=T.int32, device=dev)
        h.check(h.L.avsim_jpeg_decode(h.h, d_buf.data_ptr(), buf.shape[1], d_len.data_ptr(), None, 6, H, W, fmt, 0, whole.data_ptr() + GUARD, st.data_ptr()))
        assert st.cpu().numpy().tolist() == want
        o = whole.cpu().numpy()
        assert (o[:GUARD] == 0xAA).all() and (o[GUARD + 6 * slot:] == 0xAA).all()
        for i, ref in good.items():
            got = o[GUARD + i * slot:GUARD + (i + 1) * slot]
            if fmt == 0:
                assert np.array_equal(got.reshape(H, W, 3), ref), i
            else:
                assert T.equal(T.from_numpy(got.view(np.float32).reshape(3, H, W)), T.from_numpy(ref).permute(2, 0, 1).float() / 255), i
        # one call per image into slots with gaps
        gapped = T.full((6 * (GUARD + slot) + GUARD,), 0xAA, dtype=T.uint8, device=dev)
        idx = T.arange(6, dtype=T.int32, device=dev)
        for i in range(6):
            h.check(h.L.avsim_jpeg_decode(h.h, d_buf.data_ptr(), buf.shape[1], d_len.data_ptr(), idx[i:].data_ptr(), 1, H, W, fmt, 1,
                                          gapped.data_ptr() + GUARD + i * (GUARD + slot), st[i:].data_ptr()))
        assert st.cpu().numpy().tolist() == want
        g = gapped.cpu().numpy().reshape(-1)
        for i in range(7):
            assert (g[i * (GUARD + slot):i * (GUARD + slot) + GUARD] == 0xAA).all(), i
        if fmt == 0:
            for i in good:
                assert np.array_equal(g[GUARD + i * (GUARD + slot):][:slot].reshape(H, W, 3), jpeg.decode_reference(streams[i], "triangle")), i
    h.close()
    # the host layer raises with the first flagged stream's status
    s = BatchedSim("insert_peg", 3, 2)
    with pytest.raises(jpeg.JpegError) as e:
        s.decode_jpeg([streams[0], streams[3]])
    assert e.value.status == jpeg.STATUS_HEADER
    s.close()


def test_vec_env_round_trip():
    kw = dict(cameras=["zed_cam_left"], seed=3, observation_height=120, observation_width=160)
    for fmt in ("lerobot", "gym"):
        env = make_vec(PEG, 4, 12, obs_format=fmt, **kw)
        env.reset()
        buf, ln = env.encode_jpeg("zed_cam_left", quality=90)
        img, st = env.decode_jpeg(buf, ln)
        tri, st2 = env.decode_jpeg(buf, ln, upsample="triangle", fmt="gym")
        b, l = buf.cpu().numpy(), ln.cpu().numpy()
        assert not st.cpu().numpy().any() and not st2.cpu().numpy().any()
        for i in range(4):
            stream = b[i, :l[i]].tobytes()
            want = T.from_numpy(jpeg.decode_reference(stream))
            if fmt == "lerobot":
                assert img.dtype == T.float32 and T.equal(img[i].cpu(), want.permute(2, 0, 1).float() / 255), i
            else:
                assert img.dtype == T.uint8 and T.equal(img[i].cpu(), want), i
            assert np.array_equal(tri[i].cpu().numpy(), jpeg.decode_reference(stream, "triangle")), i
        env.close()


def test_recorded_compressed_episodes_feed_the_dataset(tmp_path):
    """harness.record_scripted(jpeg_quality=) -> episode files in the compressed layout -> dataset.CompressedDataset batches on the device.
    One wrist camera is the smallest camera set of the Cartesian env (480 x 640; the ZED pair is 720 x 1440).  The specification decodes a
    few frames only: it is a Python loop per coefficient."""
    from av_aloha_amd import harness
    from av_aloha_amd.dataset import CompressedDataset
    cam, H, W = "cam_right_wrist", 480, 640
    eps = harness.record_scripted("sim_insert_peg", 2, cameras=[cam], jpeg_quality=90, stream_dir=str(tmp_path), seed=11, keep_diverged=True)
    paths = [e["path"] for e in eps]
    assert [os.path.basename(p) for p in paths] == ["episode_0.hdf5", "episode_1.hdf5"]
    plain = [harness.load_episode(p) for p in paths]
    tsteps = eps[0]["steps"]
    table, ln = plain[0][f"/observations/images/{cam}"], plain[0]["/compress_len"]
    assert table.dtype == np.uint8 and table.ndim == 2 and table.shape == (tsteps, int(ln.max())) and ln.dtype == np.int32 and ln.shape == (1, tsteps)
    assert plain[0]["/action"].shape == (tsteps, 21) and plain[0]["/observations/all_qpos"].shape[0] == tsteps
    raw = harness._image_bytes_per_step([cam]) * tsteps
    assert raw == H * W * 3 * tsteps and os.path.getsize(paths[0]) * 10 < raw, (os.path.getsize(paths[0]), raw)
    streams = [harness.episode_streams(d)[cam] for d in plain]
    assert jpeg.stream_size(streams[0][0]) == (H, W)
    ds = CompressedDataset(paths, [cam])
    assert len(ds) == 2 * tsteps
    frames = ((0, 0), (0, 1), (0, tsteps - 1), (1, 0))
    batch = ds.batch([0, 1, tsteps - 1, tsteps])
    assert batch["episode_index"].cpu().tolist() == [e for e, _ in frames] and batch["frame_index"].cpu().tolist() == [t for _, t in frames]
    assert batch["episode_index"].dtype == batch["frame_index"].dtype == T.int64
    img = batch[f"observation.images.{cam}"]
    assert img.dtype == T.float32 and tuple(img.shape) == (4, 3, H, W) and img.device.type == "cuda"
    host = {f: jpeg.decode_reference(streams[f[0]][f[1]]) for f in frames[1:]}
    for k, f in enumerate(frames):
        if f in host:
            assert T.equal(img[k].cpu(), T.from_numpy(host[f]).permute(2, 0, 1).float() / 255), f
    assert host[(0, 1)].std() > 5 and not np.array_equal(host[(0, 1)], host[(0, tsteps - 1)])          # pictures, and the arm moved
    for key, src in (("observation.state", "/observations/qpos"), ("action", "/action")):
        assert batch[key].dtype == T.float32 and tuple(batch[key].shape) == (4, 21) and batch[key].device.type == "cuda"
        assert np.array_equal(batch[key].cpu().numpy(), np.stack([plain[e][src][t] for e, t in frames]))
    seen = T.cat([b["episode_index"] * tsteps + b["frame_index"] for b in ds.batches(256, seed=1)]).cpu().numpy()
    assert sorted(seen.tolist()) == list(range(2 * tsteps)) and seen.tolist() != list(range(2 * tsteps))
    ds.close()
    # a whole file through the device (load_episode(decode=BatchedSim)) holds the frames the specification and the data set give
    s = BatchedSim("insert_peg", 3, 2)
    dev = harness.load_episode(paths[1], decode=s)
    s.close()
    stack = dev[f"/observations/images/{cam}"]
    assert "/compress_len" not in dev and stack.dtype == np.uint8 and stack.shape == (tsteps, H, W, 3)
    assert np.array_equal(stack[0], host[(1, 0)])
    assert T.equal(T.from_numpy(stack[0]).permute(2, 0, 1).float() / 255, img[3].cpu())
