"""dataset.TrainingBatches with a config that has the geometric op (imgaug.LEROBOT_CFG) against its numpy assembly:
imgaug.jitter_affine_reference applied to the decoded u8 frames (jpeg.decode_reference) with plan(epoch)'s boxes and augment_plan(epoch)'s
masks, factors and matrices; with n_obs_steps, one matrix per item over its K frames; and augment=True, which has no such op, against the
assembly it had.  A tiny data set written by the package's own writer: two episodes of 2 and 9 frames, two cameras of 16 x 24 and 24 x 32
random pixels.  Images are compared with np.array_equal (no NaN in either)."""
import numpy as np
import pytest

from av_aloha_amd import dataset, harness, imgaug, imgprep, jpeg
from avsim_test_util import bits
import gpu_util          # noqa: F401  (torch's HIP runtime comes up before libavsim's)

pytestmark = pytest.mark.gpu

CAMS = {"cam_a": (16, 24), "cam_b": (24, 32)}
LENS = (2, 9)
CROP = (12, 20)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The episode files, the data set on the device and the decoded frames (computed once, shared, never changed)."""
    root = tmp_path_factory.mktemp("tiny_affine")
    rng = np.random.default_rng(16)
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


def affine_cfg(interpolation):
    """LEROBOT_CFG with wider ranges, so that images of 16 x 24 pixels move by more than a pixel."""
    return dict(imgaug.LEROBOT_CFG, affine={"degrees": (-15, 15), "translate": (0.2, 0.2), "interpolation": interpolation})


@pytest.mark.parametrize("normalise", [True, False])
def test_lerobot_cfg_epochs_equal_their_numpy_assembly(data, normalise):
    ds, frames, st = data
    seed = 11
    for cfg, interp in ((imgaug.LEROBOT_CFG, 0), (affine_cfg("bilinear"), 1)):
        tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, normalise=normalise, augment=cfg)
        plain = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, normalise=normalise)
        seen = 0
        for epoch in range(2):
            got, base = list(tb), list(plain)
            plan, aug = tb.plan(epoch), tb.augment_plan(epoch)
            assert len(got) == len(plan) == len(aug) == len(base) == 2
            for b, (g, p, (part, boxes), a) in enumerate(zip(got, base, plan, aug)):
                assert set(g) == set(p)
                for k in set(g) - {f"observation.images.{c}" for c in CAMS}:      # state, action, action_is_pad, the indices: untouched
                    assert g[k].dtype == p[k].dtype and np.array_equal(g[k].cpu().numpy().view(np.uint8), p[k].cpu().numpy().view(np.uint8)), k
                for ci, (c, size) in enumerate(CAMS.items()):
                    mask, fac, mat = a[c]
                    m2, f2, a2, _ = imgaug.augment_plan_affine(5, cfg, seed, epoch, b, ci, size=size)
                    assert np.array_equal(mask, m2) and np.array_equal(bits(fac), bits(f2)) and np.array_equal(bits(mat), bits(a2)) and mat.shape == (5, 6)
                    seen += int((mask & 32).astype(bool).sum())
                    s = st[f"observation.images.{c}"]
                    want = imgaug.jitter_affine_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), mat, interp, CROP,
                                                          *((s["mean"], s["std"]) if normalise else (None, None)))
                    img = g[f"observation.images.{c}"].cpu().numpy()
                    assert img.dtype == np.float32 and not np.isnan(img).any() and not np.isnan(want).any() and np.array_equal(img, want), (epoch, b, c)
        assert seen >= 10                                                       # about half of the 40 images had the op


def test_a_history_shares_one_matrix_per_item(data):
    ds, frames, st = data
    K, cfg = 3, affine_cfg("nearest")
    tb = dataset.TrainingBatches(ds, batch_size=4, chunk_size=3, stats=st, crop=CROP, seed=7, drop_last=False, n_obs_steps=K, augment=cfg)
    for epoch in range(2):
        got, plan, aug = list(tb), tb.plan(epoch), tb.augment_plan(epoch)
        assert [int(g["frame_index"].shape[0]) for g in got] == [4, 4, 3]
        for g, (part, boxes), a in zip(got, plan, aug):
            B = len(part)
            hidx, hpad = imgprep.history_index(ds.ep_start, ds.ep_len, part, K)
            for c in CAMS:
                mask, fac, mat = a[c]
                assert mat.shape == (B, 6)
                s = st[f"observation.images.{c}"]
                rep = lambda v: np.repeat(v, K, axis=0)
                want = imgaug.jitter_affine_reference(frames[c][hidx.reshape(-1)], imgaug.pack_params(rep(np.asarray(boxes[c]).reshape(B, 3)), rep(mask), rep(fac)), rep(mat),
                                                      0, CROP, s["mean"], s["std"]).reshape(B, K, 3, *CROP)
                img = g[f"observation.images.{c}"].cpu().numpy()
                assert not np.isnan(img).any() and np.array_equal(img, want), (epoch, c)
                assert np.array_equal(g[f"observation.images.{c}_is_pad"].cpu().numpy(), hpad)


def test_augment_true_has_not_changed_a_bit(data):
    """augment=True, a dict without affine and one with affine at weight 0: the plan of two elements, avsim_image_jitter's call, the bits of
    imgaug.jitter_reference with imgaug.augment_plan's draws."""
    ds, frames, st = data
    seed = 11
    for cfg in (True, {"affine": {"weight": 0}}):
        tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, augment=cfg)
        for epoch in range(2):
            got, plan, aug = list(tb), tb.plan(epoch), tb.augment_plan(epoch)
            for b, (g, (part, boxes), a) in enumerate(zip(got, plan, aug)):
                for ci, c in enumerate(CAMS):
                    assert len(a[c]) == 2
                    mask, fac = a[c]
                    m2, f2 = imgaug.augment_plan(5, None, seed, epoch, b, ci)
                    assert np.array_equal(mask, m2) and np.array_equal(bits(fac), bits(f2))
                    s = st[f"observation.images.{c}"]
                    want = imgaug.jitter_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), CROP, s["mean"], s["std"])
                    assert np.array_equal(bits(g[f"observation.images.{c}"].cpu().numpy()), bits(want)), (epoch, b, c)
