"""The JPEG stream of av_aloha_amd/jpeg.py (the specification of the device encoder, avsim_jpeg_encode) and the Motion-JPEG AVI container of
av_aloha_amd/mjpeg.py, on the CPU.  Pillow (libjpeg) is the independent decoder and the encoder to compare with; only tests import it.

Bounds: both encoders use the Annex K tables at the same quality, 4:2:0 and one restart interval per MCU row, so they differ only in the
rounding of colour conversion, DCT and quantiser.  Measured when the format was chosen: PSNR at most 0.023 dB below Pillow's, length 0.944 to
1.0001 of Pillow's.  Asserted: not more than 0.1 dB below (four times the worst gap) and not above 1.01 x the length (one percent for the
header difference) -- a wrong table, zigzag or rounding costs far more."""
import io
import os
import warnings

import numpy as np
import pytest

from PIL import Image

from av_aloha_amd import jpeg
from av_aloha_amd.mjpeg import AviWriter, read_avi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES = (50, 75, 90, 100)
RENDERED = ("r03_visual_zed_cam_left_480x640.png", "r05_visual_zed_cam_left_shadows_ss.png", "r05_visual_overhead_cam_shadows_ss.png")


def rendered(name):
    return np.array(Image.open(os.path.join(ROOT, "profiles", name)).convert("RGB"))


def synthetic():
    rng = np.random.default_rng(0)
    g = np.linspace(0, 255, 160).astype(np.uint8)
    return {"noise_37x53": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
            "noise_96x128": rng.integers(0, 256, (96, 128, 3), dtype=np.uint8),
            "white_32x48": np.full((32, 48, 3), 255, np.uint8),
            "ramp_120x160": np.stack([np.tile(g, (120, 1)), np.tile(g[::-1], (120, 1)), np.full((120, 160), 77, np.uint8)], -1)}


def decode(stream):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(stream))
        im.load()
        return np.array(im.convert("RGB"))


def pillow_encode(img, q):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=q, subsampling=2, restart_marker_rows=1)
    return b.getvalue()


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


def segments(stream):
    """[(marker, payload)] up to and including SOS, and the offset of the entropy-coded data."""
    assert stream[:2] == b"\xff\xd8"
    out, i = [(0xD8, b"")], 2
    while True:
        assert stream[i] == 0xFF, i
        m, n = stream[i + 1], int.from_bytes(stream[i + 2:i + 4], "big")
        out.append((m, stream[i + 4:i + 2 + n]))
        i += 2 + n
        if m == 0xDA:
            return out, i


def tables_of(stream, marker):
    """{table id: bytes} of the DQT (0xDB) / DHT (0xC4) segments, split where a segment holds several tables."""
    out = {}
    for m, p in segments(stream)[0]:
        if m != marker:
            continue
        while p:
            n = 65 if marker == 0xDB else 17 + sum(p[1:17])
            out[p[0]] = p[1:n]
            p = p[n:]
    return out


@pytest.mark.parametrize("name", RENDERED)
def test_rendered_frames_against_pillow(name):
    img = rendered(name)
    H, W, _ = img.shape
    for q in QUALITIES:
        ours, theirs = jpeg.encode_reference(img, q), pillow_encode(img, q)
        dec = decode(ours)
        assert dec.shape == img.shape and len(ours) <= jpeg.bound(H, W)
        p_ours, p_theirs = psnr(img, dec), psnr(img, decode(theirs))
        print(f"{name} q{q}: {len(ours)} B {p_ours:.3f} dB | Pillow {len(theirs)} B {p_theirs:.3f} dB | ratio {len(ours) / len(theirs):.4f}")
        assert p_ours >= p_theirs - 0.1, (name, q, p_ours, p_theirs)
        assert len(ours) <= 1.01 * len(theirs), (name, q, len(ours), len(theirs))


def test_synthetic_images_against_pillow():
    """Noise at 96 x 128 (whole MCUs) is held to the bounds of the rendered frames.  The colour ramp (120 rows: a partial MCU row, which
    Pillow pads differently) and noise at 37 x 53 are checked for decodability and size; the ramp's PSNR is printed next to Pillow's and
    bounded from reasoning alone: at quality >= 50 the quantiser steps of the low frequencies are <= 17 (Annex K), an error of a few grey
    levels on a smooth ramp, so 30 dB (an RMS error of 8 levels) is generous, and a wrong table or zigzag order lands below 20 dB."""
    for name, img in synthetic().items():
        H, W, _ = img.shape
        for q in QUALITIES:
            ours, theirs = jpeg.encode_reference(img, q), pillow_encode(img, q)
            dec = decode(ours)
            assert dec.shape == img.shape and len(ours) <= jpeg.bound(H, W), (name, q)
            if name == "white_32x48":         # no error at all on either side: equal pixels
                assert np.array_equal(dec, decode(theirs)), (name, q)
                assert len(ours) <= 1.01 * len(theirs), (name, q, len(ours), len(theirs))
                continue
            p_ours, p_theirs = psnr(img, dec), psnr(img, decode(theirs))
            print(f"{name} q{q}: {len(ours)} B {p_ours:.3f} dB | Pillow {len(theirs)} B {p_theirs:.3f} dB | ratio {len(ours) / len(theirs):.4f}")
            if name == "noise_96x128":
                assert p_ours >= p_theirs - 0.1, (name, q, p_ours, p_theirs)
                assert len(ours) <= 1.01 * len(theirs), (name, q, len(ours), len(theirs))
            elif name == "ramp_120x160":
                assert p_ours >= 30.0, (name, q, p_ours)


@pytest.mark.parametrize("q", [1, 10, 49, 50, 75, 90, 100])
def test_tables_are_the_ones_pillow_writes(q):
    ours = jpeg.encode_reference(np.zeros((16, 16, 3), np.uint8), q)
    theirs = pillow_encode(np.zeros((16, 16, 3), np.uint8), q)
    assert tables_of(ours, 0xDB) == tables_of(theirs, 0xDB)
    assert tables_of(ours, 0xC4) == tables_of(theirs, 0xC4)
    assert sorted(tables_of(ours, 0xC4)) == [0x00, 0x01, 0x10, 0x11]


def test_stream_structure():
    for name, img in synthetic().items():
        H, W, _ = img.shape
        mh, mw = (H + 15) // 16, (W + 15) // 16
        s = jpeg.encode_reference(img, 90)
        segs, start = segments(s)
        assert [m for m, _ in segs] == [0xD8, 0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
        assert s[:start] == jpeg.header(H, W, 90) and start == jpeg.HEADER_BYTES
        assert segs[1][1] == b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
        assert [p[0] for m, p in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
        sof = segs[4][1]
        assert sof[0] == 8 and int.from_bytes(sof[1:3], "big") == H and int.from_bytes(sof[3:5], "big") == W
        assert sof[5:] == bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
        assert int.from_bytes(segs[9][1], "big") == mw
        assert s[-2:] == b"\xff\xd9"
        data, rst, i = s[start:-2], [], 0
        while i < len(data):
            if data[i] == 0xFF:
                assert i + 1 < len(data) and (data[i + 1] == 0 or 0xD0 <= data[i + 1] <= 0xD7), (name, i)
                if data[i + 1]:
                    rst.append(data[i + 1] - 0xD0)
                i += 2
            else:
                i += 1
        assert rst == [r % 8 for r in range(mh - 1)], name


def test_argument_checks():
    with pytest.raises(ValueError):
        jpeg.encode_reference(np.zeros((8, 8, 3), np.uint8), 0)
    with pytest.raises(ValueError):
        jpeg.encode_reference(np.zeros((8, 8, 3), np.uint8), 101)
    with pytest.raises(ValueError):
        jpeg.encode_reference(np.zeros((8, 8, 3), np.float32), 90)
    with pytest.raises(ValueError):
        jpeg.header(0, 8, 90)
    with pytest.raises(ValueError):
        jpeg.bound(8, 65536)
    assert jpeg.bound(480, 640) == 629 + 30 * 40 * 6 * 416 + 2 * 29 + 2


def test_avi_round_trip(tmp_path):
    imgs = list(synthetic().values())
    ramp = imgs[3]
    rng = np.random.default_rng(3)
    frames = []
    for t in range(40):                                     # until frames of odd and of even length are in the file, five at least
        img = np.roll(ramp, 7 * t, axis=1)
        img[8:40, 16 + t:80 + t] = rng.integers(0, 256, (32, 64, 3), dtype=np.uint8)
        frames.append(jpeg.encode_reference(img, 75))
        if t >= 4 and any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames):
            break
    assert any(len(f) % 2 for f in frames) and any(len(f) % 2 == 0 for f in frames)
    path = str(tmp_path / "video" / "rollout_0.avi")
    os.makedirs(os.path.dirname(path))
    w = AviWriter(path, 160, 120, fps=25)
    for f in frames:
        w.add(f)
        assert os.path.exists(path + ".part") and not os.path.exists(path)
    w.close()
    assert os.path.exists(path) and not os.path.exists(path + ".part")
    info, got = read_avi(path)
    assert info == {"frames": len(frames), "width": 160, "height": 120, "fps": 25.0, "codec": "MJPG"}
    assert got == frames
    for f in got:
        assert decode(f).shape == (120, 160, 3)
    raw = open(path, "rb").read()
    assert len(raw) % 2 == 0 and int.from_bytes(raw[4:8], "little") == len(raw) - 8
    # the chunks start on even offsets: an odd frame is followed by a pad byte
    pos = raw.index(b"movi") + 4
    for f in frames:
        assert raw[pos:pos + 4] == b"00dc" and int.from_bytes(raw[pos + 4:pos + 8], "little") == len(f) and pos % 2 == 0
        pos += 8 + len(f) + len(f) % 2
    assert raw[pos:pos + 4] == b"idx1"
    # an aborted writer leaves nothing behind
    w = AviWriter(str(tmp_path / "x.avi"), 160, 120)
    w.add(frames[0])
    w.abort()
    assert not os.path.exists(str(tmp_path / "x.avi")) and not os.path.exists(str(tmp_path / "x.avi.part"))
    with pytest.raises(ValueError):
        AviWriter(str(tmp_path / "y.avi"), 160, 120).add(b"not a jpeg")


class _StubEnv:
    num_envs = 4
    cameras = ["zed_cam_left"]
    max_episode_steps = 5

    def start_log(self, *a, **k):
        raise AssertionError("the arguments are checked before the env is touched")


def test_evaluate_vec_video_argument_errors(tmp_path):
    from av_aloha_amd.harness import evaluate_vec
    with pytest.raises(ValueError, match="video_episodes"):
        evaluate_vec(_StubEnv(), None, 8, video_dir=str(tmp_path), video_episodes=5)
    with pytest.raises(ValueError, match="does not render"):
        evaluate_vec(_StubEnv(), None, 8, video_dir=str(tmp_path), video_camera="overhead_cam", video_episodes=2)
    assert os.listdir(str(tmp_path)) == []
