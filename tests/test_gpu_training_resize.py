"""dataset.TrainingBatches(resize=...) and harness.make_preprocessor(resize=...) against their numpy assembly: imgresize.resize_reference on the
decoded u8 frames (jpeg.decode_reference) with plan(epoch)'s boxes as source regions; with augment, imgaug.jitter_reference without
normalisation and then resize_reference on its floats (format 1); with n_obs_steps, one region per item over its K frames.  A tiny data set
written by the package's own writer: two episodes of 2 and 9 frames, two cameras of 16 x 24 and 24 x 32 random pixels.  Images are compared
with np.array_equal (no NaN in either)."""
import numpy as np
import pytest

from av_aloha_amd import dataset, harness, imgaug, imgprep, imgresize, jpeg
from av_aloha_amd.vec_env import make_vec
import gpu_util          # noqa: F401  (torch's HIP runtime comes up before libavsim's)

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
CAMS = {"cam_a": (16, 24), "cam_b": (24, 32)}
LENS = (2, 9)
CROP = (12, 20)
RESIZE = (24, 32)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The episode files, the data set on the device and the decoded frames (computed once, shared, never changed)."""
    root = tmp_path_factory.mktemp("tiny_resize")
    rng = np.random.default_rng(18)
    paths, frames = [], {c: [] for c in CAMS}
    for e, T in enumerate(LENS):
        ep = {"/observations/qpos": rng.standard_normal((T, 21)).astype(np.float32), "/action": rng.standard_normal((T, 21)).astype(np.float32)}
        for c, (H, W) in CAMS.items():
            ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        paths.append(harness.save_episode(ep, str(root), e, jpeg_quality=90))
        for c, ss in harness.episode_streams(harness.load_episode(paths[-1])).items():
            frames[c] += [jpeg.decode_reference(s) for s in ss]
    ds = dataset.CompressedDataset(paths, list(CAMS))
    yield ds, {c: np.stack(v) for c, v in frames.items()}, ds.stats()
    ds.close()


def same_image(got, want, what):
    img = got.cpu().numpy()
    assert img.dtype == np.float32 and img.shape == want.shape and not np.isnan(img).any() and not np.isnan(want).any() and np.array_equal(img, want), what


# the issue's case -- the 12 x 20 crop letterboxed into 24 x 32, an enlargement --, and the whole frame squeezed to 7 x 9, plain and not normalised
CONFIGS = [dict(crop=CROP, resize=RESIZE, resize_mode="pad"), dict(crop=None, resize=(7, 9), resize_mode="stretch", antialias=False, normalise=False),
           dict(crop=CROP, resize=(5, 6), resize_mode="pad", crop_mode="center")]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["pad-24x32", "stretch-7x9", "pad-5x6"])
def test_epochs_equal_their_numpy_assembly(data, cfg):
    ds, frames, st = data
    kw = dict(cfg)
    tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, seed=11, **kw)
    plain = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, seed=11, **{k: v for k, v in kw.items() if k not in ("resize", "resize_mode", "antialias")})
    for epoch in range(2):
        got, base, plan = list(tb), list(plain), tb.plan(epoch)
        assert len(got) == len(plan) == len(base) == 2
        for g, p, (part, boxes), (part0, boxes0) in zip(got, base, plan, plain.plan(epoch)):
            assert np.array_equal(part, part0) and set(g) == set(p)
            for k in set(g) - {f"observation.images.{c}" for c in CAMS}:      # state, action, action_is_pad, the indices: untouched
                assert g[k].dtype == p[k].dtype and np.array_equal(g[k].cpu().numpy().view(np.uint8), p[k].cpu().numpy().view(np.uint8)), k
            for c, size in CAMS.items():
                assert np.array_equal(boxes[c], boxes0[c])
                s = st[f"observation.images.{c}"]
                sb, dst = imgresize.boxes(boxes[c], kw["crop"] or size, kw["resize"], kw["resize_mode"])
                want = imgresize.resize_reference(frames[c][part], 0, sb, dst, kw["resize"], int(kw.get("antialias", True)), None,
                                                  *((s["mean"], s["std"]) if kw.get("normalise", True) else (None, None)))
                assert want.shape == (5, 3, *kw["resize"])
                same_image(g[f"observation.images.{c}"], want, (epoch, c))
    if cfg is CONFIGS[0]:          # the letterbox: 12 x 20 -> 19 x 32 under five rows of normalised zeros
        assert tuple(dst[0]) == (0, 5, 32, 19)
        s = st["observation.images.cam_b"]
        zero = (np.zeros(3, dtype=np.float32) - s["mean"].reshape(3)) / s["std"].reshape(3)
        assert np.array_equal(got[-1]["observation.images.cam_b"].cpu().numpy()[:, :, :5], np.broadcast_to(zero.reshape(1, 3, 1, 1), (5, 3, 5, 32)))


def test_with_augment_the_floats_are_resized(data):
    ds, frames, st = data
    seed = 12
    tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, augment=True, resize=RESIZE, resize_mode="pad")
    for epoch in range(2):
        got, plan, aug = list(tb), tb.plan(epoch), tb.augment_plan(epoch)
        for b, (g, (part, boxes), a) in enumerate(zip(got, plan, aug)):
            for ci, c in enumerate(CAMS):
                mask, fac = a[c]
                m2, f2 = imgaug.augment_plan(5, None, seed, epoch, b, ci)
                assert np.array_equal(mask, m2) and np.array_equal(fac.view(np.uint32), f2.view(np.uint32))
                s = st[f"observation.images.{c}"]
                floats = imgaug.jitter_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), CROP, None, None)
                sb, dst = imgresize.boxes(np.zeros((5, 3), dtype=np.int32), CROP, RESIZE, "pad")
                want = imgresize.resize_reference(floats, 1, sb, dst, RESIZE, 1, None, s["mean"], s["std"])
                same_image(g[f"observation.images.{c}"], want, (epoch, b, c))
    # an affine config goes the same way
    cfg = dict(imgaug.LEROBOT_CFG, affine={"degrees": (-15, 15), "translate": (0.2, 0.2), "interpolation": "bilinear"})
    tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, augment=cfg, resize=(6, 10))
    g, (part, boxes), a = next(iter(tb)), tb.plan(0)[0], tb.augment_plan(0)[0]
    for c in CAMS:
        mask, fac, mat = a[c]
        s = st[f"observation.images.{c}"]
        floats = imgaug.jitter_affine_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), mat, 1, CROP, None, None)
        sb, dst = imgresize.boxes(np.zeros((5, 3), dtype=np.int32), CROP, (6, 10), "stretch")
        same_image(g[f"observation.images.{c}"], imgresize.resize_reference(floats, 1, sb, dst, (6, 10), 1, None, s["mean"], s["std"]), c)


@pytest.mark.parametrize("augment", [None, True], ids=["plain", "augment"])
def test_a_history_shares_one_region_per_item(data, augment):
    ds, frames, st = data
    K = 2
    tb = dataset.TrainingBatches(ds, batch_size=4, chunk_size=3, stats=st, crop=CROP, seed=7, drop_last=False, n_obs_steps=K, augment=augment, resize=RESIZE, resize_mode="pad")
    got, plan = list(tb), tb.plan(0)
    aug = tb.augment_plan(0) or [None] * len(plan)
    assert [int(g["frame_index"].shape[0]) for g in got] == [4, 4, 3]
    for g, (part, boxes), a in zip(got, plan, aug):
        B = len(part)
        hidx, hpad = imgprep.history_index(ds.ep_start, ds.ep_len, part, K)
        rep = lambda v: np.repeat(v, K, axis=0)
        for c in CAMS:
            s = st[f"observation.images.{c}"]
            box = rep(np.asarray(boxes[c]).reshape(B, 3))
            src, fmt = frames[c][hidx.reshape(-1)], 0
            if a is not None:
                src, fmt = imgaug.jitter_reference(src, imgaug.pack_params(box, rep(a[c][0]), rep(a[c][1])), CROP, None, None), 1
                box = np.zeros((B * K, 3), dtype=np.int32)
            sb, dst = imgresize.boxes(box, CROP, RESIZE, "pad")
            want = imgresize.resize_reference(src, fmt, sb, dst, RESIZE, 1, None, s["mean"], s["std"]).reshape(B, K, 3, *RESIZE)
            same_image(g[f"observation.images.{c}"], want, c)
            assert np.array_equal(g[f"observation.images.{c}_is_pad"].cpu().numpy(), hpad)


@pytest.mark.parametrize("fmt", ["lerobot", "gym"])
def test_preprocessor_resizes_as_training_does(fmt):
    """make_preprocessor(resize=...) on the env's own frames equals what TrainingBatches(crop_mode="center", resize=...) makes of the same
    frame: resize_reference on its u8 pixels with the centred box as the region."""
    cam, H, W, crop, resize = "zed_cam_left", 48, 64, (40, 52), (24, 24)
    env = make_vec(PEG, num_envs=2, max_episode_steps=5, cameras=[cam], obs_format=fmt, observation_height=H, observation_width=W)
    try:
        obs, _ = env.reset(seed=3)
        D = env.nj
        rng = np.random.default_rng(8)
        st = {f"observation.images.{cam}": {"mean": np.array([0.4, 0.5, 0.6], np.float32).reshape(3, 1, 1), "std": np.array([0.2, 0.25, 0.3], np.float32).reshape(3, 1, 1)},
              "observation.state": {"mean": rng.standard_normal(D).astype(np.float32), "std": (1 + rng.random(D)).astype(np.float32)}}
        s = st[f"observation.images.{cam}"]
        u8 = imgprep.to_u8(env.camera_images(cam).cpu().numpy())
        assert u8.std() > 0
        x0, y0 = imgprep.center_box((H, W), crop)
        for mode, antialias in (("pad", True), ("stretch", False)):
            pre = harness.make_preprocessor(env, st, crop=crop, resize=resize, resize_mode=mode, antialias=antialias)
            got = pre(obs)
            boxes = dataset.epoch_plan(2, 2, {cam: (H, W)}, crop, "center")[0][1][cam]
            assert [tuple(b) for b in boxes] == [(x0, y0, 0)] * 2
            sb, dst = imgresize.boxes(boxes, crop, resize, mode)
            if mode == "pad":
                assert tuple(dst[0]) == (0, 6, 24, 18)
            want = imgresize.resize_reference(u8, 0, sb, dst, resize, int(antialias), None, s["mean"], s["std"])
            same_image(got[f"observation.images.{cam}"], want, (fmt, mode))
            state = (obs["observation.state"] if fmt == "lerobot" else obs["agent_pos"]).cpu().numpy().astype(np.float32)
            assert np.array_equal(got["observation.state"].cpu().numpy(), (state - st["observation.state"]["mean"]) / st["observation.state"]["std"])
            assert set(got) == {f"observation.images.{cam}", "observation.state"}
        with pytest.raises(ValueError):
            harness.make_preprocessor(env, st, crop=crop, resize=(2, 24))          # 40 rows -> 2: above the ratio cap
        with pytest.raises(ValueError):
            harness.history_preprocessor(env, st, crop=crop, n_obs_steps=2, resize=resize)
        with pytest.raises(ValueError):
            env.resize_images(env.camera_images(cam), [(0, 0, W, H + 1, 0)] * 2, [(0, 0, 24, 24)] * 2, resize)
    finally:
        env.close()
