"""dataset.CompressedDataset.stats, dataset.TrainingBatches and harness.make_preprocessor against their numpy assembly: the specifications
jpeg.decode_reference, imgprep.stats_reference / combine_stats / prep_reference / chunk_index and the documented draw order
(dataset.epoch_plan).  A tiny data set written by the package's own writer: two episodes of 5 and 7 frames, two cameras of 16 x 24 and
24 x 32 random pixels.  Every comparison is for equality, floats as uint32 bit patterns."""
import numpy as np
import pytest

from av_aloha_amd import dataset, harness, imgprep, jpeg
from av_aloha_amd.vec_env import make_vec
from avsim_test_util import bits
from gpu_util import torch

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
CAMS = {"cam_a": (16, 24), "cam_b": (24, 32)}
LENS = (5, 7)
CROP = (12, 20)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The episode files, the data set on the device and the specification's view of it (computed once, shared, never changed)."""
    root = tmp_path_factory.mktemp("tiny")
    rng = np.random.default_rng(5)
    paths, frames, state, action = [], {c: [] for c in CAMS}, [], []
    for e, T in enumerate(LENS):
        ep = {"/observations/qpos": rng.standard_normal((T, 21)).astype(np.float32), "/action": rng.standard_normal((T, 21)).astype(np.float32)}
        for c, (H, W) in CAMS.items():
            ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        paths.append(harness.save_episode(ep, str(root), e, jpeg_quality=90))
        loaded = harness.load_episode(paths[-1])
        for c, ss in harness.episode_streams(loaded).items():
            frames[c] += [jpeg.decode_reference(s) for s in ss]
        state.append(ep["/observations/qpos"])
        action.append(ep["/action"])
    ds = dataset.CompressedDataset(paths, list(CAMS))
    ref = {"frames": {c: np.stack(v) for c, v in frames.items()}, "state": np.concatenate(state), "action": np.concatenate(action),
           "episode": np.repeat(np.arange(len(LENS)), LENS), "frame": np.concatenate([np.arange(T) for T in LENS])}
    yield ds, ref, root
    ds.close()


def same_stats(a, b):
    assert set(a) == set(b)
    for k in a:
        assert set(a[k]) == {"mean", "std", "min", "max"} == set(b[k])
        for n in a[k]:
            assert a[k][n].dtype == np.float32 and a[k][n].shape == b[k][n].shape and np.array_equal(bits(a[k][n]), bits(b[k][n])), (k, n)


def test_stats_equal_the_specification(data):
    ds, ref, root = data
    st = ds.stats()
    for c, (H, W) in CAMS.items():
        want = imgprep.combine_stats(imgprep.stats_reference(ref["frames"][c]), H * W)
        got = st[f"observation.images.{c}"]
        for n in ("mean", "std", "min", "max"):
            assert got[n].shape == (3, 1, 1) and got[n].dtype == np.float32 and np.array_equal(bits(got[n]), bits(want[n])), (c, n)
    for key, x in (("observation.state", ref["state"]), ("action", ref["action"])):
        x = x.astype(np.float64)
        assert np.array_equal(st[key]["mean"], x.mean(0).astype(np.float32)) and np.array_equal(st[key]["std"], x.std(0).astype(np.float32))
        assert np.array_equal(st[key]["min"], x.min(0).astype(np.float32)) and np.array_equal(st[key]["max"], x.max(0).astype(np.float32))
    same_stats(st, ds.stats(batch_size=4))             # batches that cross the episodes' and the data set's boundaries
    path = dataset.save_stats(st, str(root / "stats.json"))
    same_stats(st, dataset.load_stats(path))


def assemble(ref, st, part, boxes, chunk, crop):
    """The batch of the frames `part` in numpy."""
    out = {"observation.state": (ref["state"][part] - st["observation.state"]["mean"]) / st["observation.state"]["std"],
           "episode_index": ref["episode"][part], "frame_index": ref["frame"][part]}
    starts = np.concatenate([[0], np.cumsum(LENS)[:-1]])
    index, pad = imgprep.chunk_index(starts, LENS, part, chunk)
    out["action"] = (ref["action"][index] - st["action"]["mean"]) / st["action"]["std"]
    out["action_is_pad"] = pad
    for c in CAMS:
        s = st[f"observation.images.{c}"]
        out[f"observation.images.{c}"] = imgprep.prep_reference(ref["frames"][c][part], imgprep.normalise_lut(s["mean"], s["std"])[None], None, boxes[c], crop)
    return out


def same_batch(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.shape == w.shape, k
        if w.dtype == np.float32:
            assert g.dtype == np.float32 and np.array_equal(bits(g), bits(w)), k
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), k


def test_an_epoch_equals_its_numpy_assembly(data):
    ds, ref, _ = data
    st = ds.stats()
    tb = dataset.TrainingBatches(ds, batch_size=5, chunk_size=4, stats=st, crop=CROP, seed=7)
    for epoch in range(2):
        got = list(tb)                                # (nothing waits for the device until the batches are read below)
        plan = dataset.epoch_plan(12, 5, CAMS, CROP, "random", seed=7, epoch=epoch)
        assert len(got) == len(plan) == len(tb) == 2  # drop_last: the two frames left over are dropped
        for g, (part, boxes) in zip(got, plan):
            assert tuple(g["action"].shape) == (5, 4, 21) and tuple(g["observation.images.cam_b"].shape) == (5, 3, 12, 20)
            same_batch(g, assemble(ref, st, part, boxes, 4, CROP))
    keep = dataset.TrainingBatches(ds, batch_size=5, chunk_size=9, stats=st, crop=CROP, crop_mode="center", seed=7, drop_last=False)
    got = list(keep)
    plan = dataset.epoch_plan(12, 5, CAMS, CROP, "center", seed=7, epoch=0, drop_last=False)
    assert [int(g["frame_index"].shape[0]) for g in got] == [5, 5, 2] and len(keep) == 3
    for g, (part, boxes) in zip(got, plan):
        same_batch(g, assemble(ref, st, part, boxes, 9, CROP))
    assert any(g["action_is_pad"].any().item() for g in got)
    # no crop, no normalisation: the decoder's float image
    plain = next(iter(dataset.TrainingBatches(ds, batch_size=3, chunk_size=1, stats=st, normalise=False, crop_mode="center", seed=1)))
    part = dataset.epoch_plan(12, 3, CAMS, None, "center", seed=1)[0][0]
    for c in CAMS:
        want = np.transpose(ref["frames"][c][part], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)
        assert np.array_equal(bits(plain[f"observation.images.{c}"].cpu().numpy()), bits(want))
    assert np.array_equal(plain["observation.state"].cpu().numpy(), ref["state"][part])
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 5, 4, st, crop=(17, 20))        # taller than cam_a
    # batch()'s default is what it was: float32 CHW in [0, 1]
    b = ds.batch([0, 11])
    want = np.transpose(ref["frames"]["cam_a"][[0, 11]], (0, 3, 1, 2)).astype(np.float32) / np.float32(255)
    assert np.array_equal(bits(b["observation.images.cam_a"].cpu().numpy()), bits(want))
    assert np.array_equal(ds.batch([0, 11], fmt="gym")["observation.images.cam_a"].cpu().numpy(), ref["frames"]["cam_a"][[0, 11]])


@pytest.mark.parametrize("fmt", ["lerobot", "gym"])
def test_preprocessor_feeds_a_policy_what_training_saw(fmt):
    cam, H, W, crop = "zed_cam_left", 48, 64, (40, 52)
    env = make_vec(PEG, num_envs=2, max_episode_steps=5, cameras=[cam], obs_format=fmt, observation_height=H, observation_width=W)
    try:
        obs, _ = env.reset(seed=3)
        D = env.nj
        rng = np.random.default_rng(8)
        st = {f"observation.images.{cam}": {"mean": np.array([0.4, 0.5, 0.6], np.float32).reshape(3, 1, 1), "std": np.array([0.2, 0.25, 0.3], np.float32).reshape(3, 1, 1)},
              "observation.state": {"mean": rng.standard_normal(D).astype(np.float32), "std": (1 + rng.random(D)).astype(np.float32)}}
        pre = harness.make_preprocessor(env, st, crop=crop)
        got = pre(obs)
        src = env.camera_images(cam).cpu().numpy()
        s = st[f"observation.images.{cam}"]
        x0, y0 = imgprep.center_box((H, W), crop)
        assert (x0, y0) == (6, 4)
        want = imgprep.prep_reference(src, imgprep.normalise_lut(s["mean"], s["std"])[None], None, [(x0, y0, 0)] * 2, crop)
        assert np.array_equal(bits(got[f"observation.images.{cam}"].cpu().numpy()), bits(want))
        state = (obs["observation.state"] if fmt == "lerobot" else obs["agent_pos"]).cpu().numpy().astype(np.float32)
        assert np.array_equal(bits(got["observation.state"].cpu().numpy()), bits((state - st["observation.state"]["mean"]) / st["observation.state"]["std"]))
        assert set(got) == {f"observation.images.{cam}", "observation.state"}
        # VecEnv.image_stats on the same buffer, whole and through an index tensor
        sums = env.image_stats(env.camera_images(cam)).cpu().numpy().view(np.uint64)
        assert np.array_equal(sums, imgprep.stats_reference(src))
        index = torch.tensor([1, 1, 0], dtype=torch.int32, device=env.device)
        assert np.array_equal(env.image_stats(env.camera_images(cam), index).cpu().numpy().view(np.uint64), imgprep.stats_reference(src, [1, 1, 0]))
        with pytest.raises(ValueError):
            env.prep_images(env.camera_images(cam), torch.zeros((1, 3, 256), device=env.device), [(13, 0, 0)], crop)
    finally:
        env.close()
