"""dataset.TrainingBatches(augment=...) against its numpy assembly: imgaug.jitter_reference applied to the decoded u8 frames
(jpeg.decode_reference) with plan(epoch)'s boxes and augment_plan(epoch)'s parameters; without augment, imgprep.prep_reference as before.  A
tiny data set written by the package's own writer: two episodes of 5 and 7 frames, two cameras of 16 x 24 and 24 x 32 random pixels.  Images
are compared with np.array_equal (no NaN in either), everything else for equality."""
import numpy as np
import pytest

from av_aloha_amd import dataset, harness, imgaug, imgprep, jpeg
from avsim_test_util import bits
import gpu_util          # noqa: F401  (torch's HIP runtime comes up before libavsim's)

pytestmark = pytest.mark.gpu

CAMS = {"cam_a": (16, 24), "cam_b": (24, 32)}
LENS = (5, 7)
CROP = (12, 20)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The episode files, the data set on the device and the decoded frames (computed once, shared, never changed)."""
    root = tmp_path_factory.mktemp("tiny_aug")
    rng = np.random.default_rng(15)
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


def image_keys():
    return [f"observation.images.{c}" for c in CAMS]


def test_without_augment_the_batches_are_what_they_were(data):
    ds, frames, st = data
    for kw in (dict(), dict(augment=None)):
        tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=7, **kw)
        assert tb.augment_plan(0) is None
        got = list(tb)
        plan = dataset.epoch_plan(12, 5, CAMS, CROP, "random", seed=7, epoch=0)
        assert len(got) == len(plan) == 2
        for g, (part, boxes) in zip(got, plan):
            for c in CAMS:
                s = st[f"observation.images.{c}"]
                want = imgprep.prep_reference(frames[c][part], imgprep.normalise_lut(s["mean"], s["std"])[None], None, boxes[c], CROP)
                assert np.array_equal(bits(g[f"observation.images.{c}"].cpu().numpy()), bits(want)), c


@pytest.mark.parametrize("normalise", [True, False])
def test_augmented_epochs_equal_their_numpy_assembly(data, normalise):
    ds, frames, st = data
    seed = 11
    tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, normalise=normalise, augment=True)
    plain = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, normalise=normalise)
    twin = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=seed, normalise=normalise, augment={})
    epochs = []
    for epoch in range(2):
        got, base, again = list(tb), list(plain), list(twin)
        plan, aug = tb.plan(epoch), tb.augment_plan(epoch)
        assert len(got) == len(plan) == len(aug) == len(base) == 2
        for b, (g, p, (part, boxes), a) in enumerate(zip(got, base, plan, aug)):
            assert set(g) == set(p)
            for k in set(g) - set(image_keys()):                       # state, action, action_is_pad, the indices: untouched
                assert g[k].dtype == p[k].dtype and np.array_equal(g[k].cpu().numpy().view(np.uint8), p[k].cpu().numpy().view(np.uint8)), k
            for ci, c in enumerate(CAMS):
                mask, fac = a[c]
                m2, f2 = imgaug.augment_plan(5, None, seed, epoch, b, ci)
                assert np.array_equal(mask, m2) and np.array_equal(bits(fac), bits(f2))
                s = st[f"observation.images.{c}"]
                want = imgaug.jitter_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), CROP, *((s["mean"], s["std"]) if normalise else (None, None)))
                img = g[f"observation.images.{c}"].cpu().numpy()
                assert img.dtype == np.float32 and not np.isnan(img).any() and not np.isnan(want).any() and np.array_equal(img, want), (epoch, b, c)
                assert not np.array_equal(img, p[f"observation.images.{c}"].cpu().numpy())
                assert np.array_equal(bits(img), bits(again[b][f"observation.images.{c}"].cpu().numpy()))      # two iterators, one seed
        epochs.append(got)
    assert not np.array_equal(epochs[0][0]["observation.images.cam_a"].cpu().numpy(), epochs[1][0]["observation.images.cam_a"].cpu().numpy())
    assert not np.array_equal(tb.augment_plan(0)[0]["cam_a"][1], tb.augment_plan(1)[0]["cam_a"][1])


def test_a_cfg_dict_overrides_fields(data):
    ds, frames, st = data
    cfg = {"max_num_transforms": 1, "hue": {"weight": 0}, "sharpness": {"min_max": (0.0, 2.0)}}
    tb = dataset.TrainingBatches(ds, batch_size=4, chunk_size=2, stats=st, crop=None, crop_mode="center", seed=3, augment=cfg, drop_last=False)
    got, plan, aug = list(tb), tb.plan(0), tb.augment_plan(0)
    assert [int(g["frame_index"].shape[0]) for g in got] == [4, 4, 4]
    for g, (part, boxes), a in zip(got, plan, aug):
        for c, (H, W) in CAMS.items():
            mask, fac = a[c]
            assert all(bin(int(m)).count("1") == 1 for m in mask) and not (mask & imgaug.HUE).any()
            s = st[f"observation.images.{c}"]
            want = imgaug.jitter_reference(frames[c][part], imgaug.pack_params(boxes[c], mask, fac), (H, W), s["mean"], s["std"])
            assert np.array_equal(g[f"observation.images.{c}"].cpu().numpy(), want)
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 4, 2, st, augment={"hue": {"min_max": (-1, 1)}})
