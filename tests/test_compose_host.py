"""The specification of the device's composer, av_aloha_amd/compose.py, against independent implementations: resize_reference against
Pillow's antialiased bilinear resize (byte equality), the layouts against the reference script's numbers written out, label_reference
against an ASCII drawing, and the two harness functions built on them through their host path (device="host").  The device is held to
this specification in tests/test_gpu_compose.py."""
import os

import numpy as np
import pytest

from av_aloha_amd import compose, harness, jpeg, mjpeg

# (input H, W) -> (output H, W)
SIZE_PAIRS = [((480, 640), (60, 80)), ((480, 640), (240, 320)), ((720, 1440), (480, 960)), ((17, 23), (5, 7)), ((17, 23), (40, 51)),
              ((480, 640), (480, 640)), ((33, 65), (32, 64)), ((9, 9), (1, 1)), ((480, 640), (97, 131)), ((64, 48), (64, 20)), ((64, 48), (30, 48))]

EPISODE_12 = """
#####.####...###...####..###..###...#####.........#....###..
#.....#...#...#...#.....#...#.#..#..#............##...#...#.
#.....#...#...#...#.....#...#.#...#.#.............#.......#.
####..####....#....###..#...#.#...#.####..........#......#..
#.....#.......#.......#.#...#.#...#.#.............#.....#...
#.....#.......#.......#.#...#.#..#..#.............#....#....
#####.#......###..####...###..###...#####........###..#####.
............................................................
"""


def art(text):
    return np.array([[ch == "#" for ch in line] for line in text.strip().splitlines()])


def noise(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(h, w):
    return np.stack([np.tile(np.linspace(0, 255, w).astype(np.uint8), (h, 1)), np.tile(np.linspace(255, 0, h).astype(np.uint8)[:, None], (1, w)),
                     np.full((h, w), 77, np.uint8)], -1)


@pytest.mark.parametrize("pair", SIZE_PAIRS, ids=lambda p: f"{p[0][0]}x{p[0][1]}-{p[1][0]}x{p[1][1]}")
def test_resize_reference_is_pillows_bilinear(pair):
    Image = pytest.importorskip("PIL.Image")
    (h, w), (oh, ow) = pair
    for name, img in (("noise", noise(h, w)), ("ramp", ramp(h, w))):
        want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
        got = compose.resize_reference(img, oh, ow)
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (name, pair, int(np.abs(got.astype(int) - want).max()))


def test_resize_reference_with_equal_sizes_returns_its_input():
    img = noise(17, 23)
    assert compose.resize_reference(img, 17, 23) is img
    half = compose.resize_reference(img, 17, 10)                  # one pass skipped: the other alone
    assert np.array_equal(half, np.stack([compose.resize_reference(np.ascontiguousarray(img[:, :, c]), 17, 10) for c in range(3)], -1))
    with pytest.raises(ValueError):
        compose.resize_reference(noise(34, 8), 2, 8)              # ratio 17


def test_axis_table_properties():
    for n_in, n_out in ((640, 80), (23, 7), (23, 51), (64, 4), (9, 1), (65, 64)):
        lo, cnt, k = compose.axis_table(n_in, n_out)
        assert k.shape[1] == 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1
        assert (lo >= 0).all() and (lo + cnt <= n_in).all() and (cnt >= 1).all() and (cnt <= k.shape[1]).all()
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + cnt) >= 0).all()
        assert (np.abs(k.sum(1) - (1 << 22)) <= 33).all() and (k >= 0).all()          # the sum stays within 2^22 + 33: int32 on the device
        assert all((k[i, cnt[i]:] == 0).all() for i in range(n_out))


def test_layout_row_gives_the_reference_numbers():
    from av_aloha_amd.env import ENVS
    spec = ENVS["gym_guided_vision/InsertPeg-3Arms-v0"]
    sizes = [(spec["observation_height"], spec["observation_width"])] * len(spec["cameras"])
    assert sizes[0] == (480, 640)
    rows, ch, cw = compose.layout_row(sizes)
    assert (ch, cw) == (480, 640 * len(sizes))
    assert rows == [(640 * i, 0, 640, 480) for i in range(len(sizes))]
    # the Cartesian env's 720 x 1440 zed_cam next to a 480 x 640 wrist camera: min_h = 480, new_w = int(480 * 1440 / 720) = 960
    rows, ch, cw = compose.layout_row([(480, 640), (720, 1440)])
    assert rows == [(0, 0, 640, 480), (640, 0, 960, 480)] and (ch, cw) == (480, 1600)
    rows, ch, cw = compose.layout_row([(720, 1440), (480, 640)])
    assert rows == [(0, 0, 960, 480), (960, 0, 640, 480)] and (ch, cw) == (480, 1600)
    rows, ch, cw = compose.layout_row([(36, 48), (24, 32)])
    assert rows == [(0, 0, 32, 24), (32, 0, 32, 24)] and (ch, cw) == (24, 64)
    rows, ch, cw = compose.layout_row([(480, 640), (481, 640)])      # int() truncates: 480 * 640 / 481 = 638.67
    assert rows[1] == (640, 0, 638, 480) and cw == 1278


def test_layout_grid():
    assert compose.layout_grid(1, 120, 160) == ([(0, 0, 160, 120)], 120, 160)
    rows, ch, cw = compose.layout_grid(5, 120, 160)                  # ceil(sqrt(5)) = 3 columns, 2 rows
    assert (ch, cw) == (240, 480)
    assert rows == [(0, 0, 160, 120), (160, 0, 160, 120), (320, 0, 160, 120), (0, 120, 160, 120), (160, 120, 160, 120)]
    rows, ch, cw = compose.layout_grid(16, 24, 32)
    assert (ch, cw) == (96, 128) and rows[5] == (32, 24, 32, 24) and rows[15] == (96, 72, 32, 24)
    rows, ch, cw = compose.layout_grid(5, 10, 20, cols=5)
    assert (ch, cw) == (10, 100) and rows[4] == (80, 0, 20, 10)


def test_compose_reference_places_and_refuses():
    src = np.stack([noise(17, 23, s) for s in range(2)])
    canvas = np.full((2, 20, 30, 3), 9, np.uint8)
    out = compose.compose_reference(canvas, src, [(0, 1, 3, 2, 7, 5), (1, 0, 7, 3, 23, 17), (0, 0, 10, 2, 7, 5)])
    assert out is canvas
    assert np.array_equal(canvas[0, 2:7, 3:10], compose.resize_reference(src[1], 5, 7))
    assert np.array_equal(canvas[0, 2:7, 10:17], compose.resize_reference(src[0], 5, 7))
    assert np.array_equal(canvas[1, 3:20, 7:30], src[0])
    mask = np.ones(canvas.shape[:3], bool)
    mask[0, 2:7, 3:17] = False
    mask[1, 3:20, 7:30] = False
    assert (canvas[mask] == 9).all()
    for bad in ([(0, 0, 24, 0, 7, 5)], [(0, 0, 0, 0, 7, 5), (0, 1, 6, 4, 7, 5)], [(0, 0, 0, 0, 7, 1)], [(0, 2, 0, 0, 7, 5)], [(2, 0, 0, 0, 7, 5)]):
        with pytest.raises(ValueError):
            compose.compose_reference(canvas.copy(), src, bad)


def test_label_reference_draws_the_ascii_art():
    want = art(EPISODE_12)
    assert want.shape == (8, 60)
    assert np.array_equal(compose.text_mask("EPISODE 12"), want)
    rng = np.random.default_rng(1)
    base = rng.integers(0, 200, (2, 40, 200, 3), dtype=np.uint8)
    for scale in (1, 3):
        big = np.repeat(np.repeat(want, scale, 0), scale, 1)         # every pixel of the drawing a scale x scale square
        canvas = base.copy()
        out = compose.label_reference(canvas, [(1, 5, 4, scale)], "EPISODE ", [12], (255, 254, 253))
        assert out is canvas
        region = np.zeros((40, 200), bool)
        region[4:4 + 8 * scale, 5:5 + 60 * scale] = big
        assert (canvas[1][region] == (255, 254, 253)).all()
        assert np.array_equal(canvas[1][~region], base[1][~region]) and np.array_equal(canvas[0], base[0])      # nothing else changes
    # the colour as 0xRRGGBB, a negative value, the prefix alone
    canvas = np.zeros((1, 8, 40, 3), np.uint8)
    compose.label_reference(canvas, [(0, 0, 0, 1)], "", [-7], 0x102030)
    assert np.array_equal(canvas[0, :, :12].any(-1), compose.text_mask("-7")) and set(map(tuple, canvas[0][canvas[0].any(-1)])) == {(0x10, 0x20, 0x30)}
    canvas = np.zeros((1, 8, 40, 3), np.uint8)
    compose.label_reference(canvas, [(0, 0, 0, 1)], "A=", None, 0xFFFFFF)
    assert np.array_equal(canvas[0, :, :12].any(-1), compose.text_mask("A=")) and not canvas[0, :, 12:].any()


def test_label_reference_unknown_characters_and_clipping():
    assert not compose.text_mask("a?_é").any()                      # no glyph: a space
    assert np.array_equal(compose.text_mask("AaB")[:, 12:], compose.text_mask("B"))
    canvas = np.zeros((1, 10, 20, 3), np.uint8)
    compose.label_reference(canvas, [(0, 14, 6, 2)], "", [88], 0xFFFFFF)          # leaves the canvas to the right and below: clipped
    m = compose.text_mask("88", 2)
    assert np.array_equal(canvas[0, 6:, 14:].any(-1), m[:4, :6])
    compose.label_reference(canvas, [(0, -3, -2, 1)], "", [4], 0xFFFFFF)          # and to the left and above
    assert np.array_equal(canvas[0, :6, :3].any(-1), compose.text_mask("4")[2:, 3:6])


def test_font_is_the_librarys_table():
    """avsim_compose_font needs no device; the Python side draws with that one copy."""
    import ctypes as C
    from av_aloha_amd.build import build_hip
    L = C.CDLL(build_hip())
    rows = np.zeros((128, 7), np.uint8)
    L.avsim_compose_font.restype = None
    L.avsim_compose_font(C.c_void_p(rows.ctypes.data))
    assert np.array_equal(rows, compose.font())
    with_glyph = {chr(c) for c in range(128) if rows[c].any()}
    assert with_glyph == set(compose.GLYPHS) - {" "}
    assert (rows < 32).all()                                         # five columns
    assert len({rows[ord(c)].tobytes() for c in with_glyph}) == len(with_glyph)          # no two glyphs alike
    want = art(EPISODE_12)
    for i, ch in enumerate("EPISODE 12"):
        cell = want[:, 6 * i:6 * i + 6]
        assert [int("".join("1" if x else "0" for x in r[:5]), 2) for r in cell[:7]] == list(rows[ord(ch)])


def synthetic_episode(seed, T=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:36, 0:48]
    smooth = np.stack([np.stack([(4 * xx + 17 * t + 40 * seed) % 256, (5 * yy + 9 * t) % 256, (xx + yy + 30 * t) % 256], -1) for t in range(T)]).astype(np.uint8)
    return {"/observations/qpos": rng.standard_normal((T, 21)).astype(np.float32), "/observations/qvel": np.zeros((T, 21), np.float32),
            "/observations/all_qpos": np.zeros((T, 30), np.float32), "/action": np.zeros((T, 21), np.float32),
            "/observations/images/cam_a": rng.integers(0, 256, (T, 24, 32, 3), dtype=np.uint8), "/observations/images/cam_b": smooth}


def expected_frames(data, number=None, prefix="EPISODE "):
    """What a frame of the video decodes to: compose_reference of the frame's images (label_reference on top) through one encode / decode."""
    out = []
    for t in range(data["/observations/images/cam_a"].shape[0]):
        canvas = np.zeros((1, 24, 64, 3), np.uint8)
        compose.compose_reference(canvas, data["/observations/images/cam_a"][t][None], [(0, 0, 0, 0, 32, 24)])
        compose.compose_reference(canvas, data["/observations/images/cam_b"][t][None], [(0, 0, 32, 0, 32, 24)])
        if number is not None:
            compose.label_reference(canvas, [(0, 10, 10, 3)], prefix, [number], 0xFFFFFF)
        out.append(jpeg.decode_reference(jpeg.encode_reference(canvas[0], 90)))
    return out


def test_visualize_episode_on_the_host(tmp_path):
    data = synthetic_episode(0)
    raw = harness.save_episode(data, str(tmp_path / "raw"), 0, use_h5py=False)
    packed = harness.save_episode(data, str(tmp_path / "packed"), 0, use_h5py=False, jpeg_quality=90)
    want = expected_frames(data)
    res = harness.visualize_episode(raw, str(tmp_path / "raw.avi"), device="host")
    assert res["frames"] == 3
    info, frames = mjpeg.read_avi(str(tmp_path / "raw.avi"))
    assert (info["frames"], info["height"], info["width"], info["fps"]) == (3, 24, 32 + 32, 50)
    for t in range(3):
        assert np.array_equal(jpeg.decode_reference(frames[t]), want[t]), t
    # the compressed file: the cameras' frames after THEIR round trip, composed
    harness.visualize_episode(packed, str(tmp_path / "packed.avi"), device="host")
    info, frames = mjpeg.read_avi(str(tmp_path / "packed.avi"))
    assert (info["frames"], info["height"], info["width"]) == (3, 24, 64)
    decoded = harness.load_episode(packed, decode="host")
    for t, w in enumerate(expected_frames(decoded)):
        assert np.array_equal(jpeg.decode_reference(frames[t]), w), t
    # one camera, every second frame, a label
    harness.visualize_episode(data, str(tmp_path / "one.avi"), cameras=["cam_b"], stride=2, label="CAM B", fps=10, device="host")
    info, frames = mjpeg.read_avi(str(tmp_path / "one.avi"))
    assert (info["frames"], info["height"], info["width"], info["fps"]) == (2, 36, 48, 10)
    canvas = data["/observations/images/cam_b"][[2]].copy()
    compose.label_reference(canvas, [(0, 10, 10, 3)], "CAM B", None, 0xFFFFFF)
    assert np.array_equal(jpeg.decode_reference(frames[1]), jpeg.decode_reference(jpeg.encode_reference(canvas[0], 90)))
    with pytest.raises(ValueError):
        harness.visualize_episode(data, str(tmp_path / "x.avi"), cameras=["cam_c"], device="host")
    assert not os.path.exists(tmp_path / "x.avi") and not os.path.exists(str(tmp_path / "x.avi") + ".part")


def test_visualize_dataset_on_the_host(tmp_path):
    eps = [synthetic_episode(1), synthetic_episode(1)]               # the same pictures twice: the frames differ by the label alone
    d = str(tmp_path / "set")
    paths = [harness.save_episode(e, d, i, use_h5py=False) for i, e in enumerate(eps)]
    res = harness.visualize_dataset(os.path.join(d, "episode_*.hdf5"), str(tmp_path / "all.avi"), stride=2, device="host")
    assert res["frames"] == 4
    info, frames = mjpeg.read_avi(str(tmp_path / "all.avi"))
    assert (info["frames"], info["height"], info["width"], info["fps"]) == (4, 24, 64, 2)          # int(1 / 0.04 / 10) = 2
    for e in range(2):
        want = expected_frames(eps[e], number=e)
        for j, t in enumerate((0, 2)):
            assert np.array_equal(jpeg.decode_reference(frames[2 * e + j]), want[t]), (e, t)
    # `EPISODE <i>` at scale 3 puts the number at x = 10 + 8 * 18, beyond this 64-column canvas: clipped, so the two episodes' frames are equal ...
    assert frames[0] == frames[2] and frames[0] != frames[1]
    # ... and with a one-letter prefix the digit's cell (x 28 .. 45, rows 10 .. 23) is on the canvas: the label pixels differ, nothing else does
    harness.visualize_dataset(paths, str(tmp_path / "short.avi"), stride=2, label="E", device="host")
    _, frames = mjpeg.read_avi(str(tmp_path / "short.avi"))
    f0, f1 = jpeg.decode_reference(frames[0]), jpeg.decode_reference(frames[2])
    assert np.array_equal(f0, expected_frames(eps[0], number=0, prefix="E")[0]) and np.array_equal(f1, expected_frames(eps[1], number=1, prefix="E")[0])
    assert (f0[:, 16:48] != f1[:, 16:48]).any()                      # the MCUs under the digit
    assert np.array_equal(f0[:, :16], f1[:, :16]) and np.array_equal(f0[:, 48:], f1[:, 48:])
    # gaps in the numbering are refused, as the reference script refuses them
    os.rename(paths[1], os.path.join(d, "episode_2.hdf5"))
    with pytest.raises(ValueError):
        harness.visualize_dataset(os.path.join(d, "episode_*.hdf5"), str(tmp_path / "gap.avi"), device="host")
