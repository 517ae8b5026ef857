"""Observation histories where they are used.

harness.chunked_policy(..., observe=...) with harness.history_preprocessor under harness.evaluate_vec: five InsertPeg envs with one 64 x 80
camera, episodes of six steps, twelve episodes.  Every call's raw observation, ids and elapsed steps are recorded, and so is every input
predict_chunk received; the specification (av_aloha_amd.obshist.ObsHistoryReference) is replayed with a push in EVERY call and every logged
input must equal it -- in queue mode the policy is skipped in most calls, the history is not.  A masked reset during the run puts two envs out
of phase (tests/test_gpu_chunked_eval.py says why it has to be during the run): their first stacked input of the new episode must hold K
copies of the reset frame.

dataset.TrainingBatches(n_obs_steps=...) against its numpy assembly (imgprep.history_index, prep_reference, imgaug.jitter_reference) on a tiny
data set with episodes of 2 and 9 frames, and against obshist.ObsHistory fed the frames of an episode in order: training and evaluation stack
alike.  Every comparison is np.array_equal on float32 arrays with no NaN on either side."""
import numpy as np
import pytest

from av_aloha_amd import dataset, harness, imgaug, imgprep, jpeg
from av_aloha_amd import obshist as oh
from av_aloha_amd.harness import chunked_policy, evaluate_vec, history_preprocessor
from av_aloha_amd.vec_env import make_vec
from avsim_test_util import same
from gpu_util import torch

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
CAM, SIZE, CROP = "zed_cam_left", (64, 80), (48, 64)
N, STEPS, EPISODES, C, K = 5, 6, 12, 4, 2
RESET_AT, RESET_ENVS = 16, (3, 4)          # the 17th select_action call: every env holds an id in 10 .. 14, envs 3 and 4 those past 11


@pytest.fixture(scope="module")
def venv():
    env = make_vec(PEG, N, STEPS, cameras=[CAM], observation_height=SIZE[0], observation_width=SIZE[1])
    yield env
    env.close()


def eval_stats(D):
    rng = np.random.default_rng(21)
    return {f"observation.images.{CAM}": {"mean": np.array([0.4, 0.5, 0.6], np.float32).reshape(3, 1, 1), "std": np.array([0.2, 0.25, 0.3], np.float32).reshape(3, 1, 1)},
            "observation.state": {"mean": (0.1 * rng.standard_normal(D)).astype(np.float32), "std": (1 + rng.random(D)).astype(np.float32)}}


def evaluate(venv, **kw):
    """-> (the history, the records of evaluate_vec, one dict per select_action call)"""
    st = eval_stats(venv.nj)
    mean = torch.from_numpy(st["observation.state"]["mean"]).to(venv.device)
    std = torch.from_numpy(st["observation.state"]["std"]).to(venv.device)
    k = torch.arange(C, dtype=torch.float32, device=venv.device)[None, :, None]
    log, calls = {}, []

    def predict_chunk(obs, info):
        """a small wave around the current joint state (the newest slot, un-normalised): inside the joint ranges"""
        log["seen"] = {key: v.cpu().numpy().copy() for key, v in obs.items()}
        state = (obs["observation.state"][:, -1] * std + mean)[:, None, :]
        return (state + 0.02 * torch.sin(0.7 * k + 0.5 * info["episode_id"][:, None, None].to(torch.float32))).contiguous()

    venv.reset(seed=3)
    mask = torch.zeros(N, dtype=torch.bool, device=venv.device)
    mask[list(RESET_ENVS)] = True
    observe, history = history_preprocessor(venv, st, crop=CROP, n_obs_steps=K)
    select, executor = chunked_policy(venv, predict_chunk, C, observe=observe, **kw)
    executor.reset()
    history.reset()

    def recording(obs, info):
        if len(calls) == RESET_AT:
            venv.reset(options={"reset_mask": mask})          # (obs and info are the env's own buffers: they now hold the new episodes)
        log["seen"] = None
        raw = {"state": obs["observation.state"].cpu().numpy().copy(), "image": venv.camera_images(CAM).cpu().numpy().copy(),
               "ids": info["episode_id"].cpu().numpy().copy(), "elapsed": info["elapsed_steps"].cpu().numpy().copy()}
        action = select(obs, info)
        calls.append({**raw, "seen": log["seen"]})
        return action
    records = evaluate_vec(venv, recording, EPISODES, seed=3)
    assert executor.starved() == 0
    return history, records, calls


def replay(history, calls):
    """the specification pushed in every call; every input the policy saw equals it.  -> the number of calls in which the policy ran"""
    ref = history.reference()
    lut = imgprep.normalise_lut([0.4, 0.5, 0.6], [0.2, 0.25, 0.3])
    x0, y0 = imgprep.center_box(SIZE, CROP)
    ran = 0
    for t, c in enumerate(calls):
        sh, ih = ref.push(c["state"], [c["image"]], c["ids"], c["elapsed"])
        if c["seen"] is None:
            continue
        ran += 1
        assert set(c["seen"]) == {"observation.state", f"observation.images.{CAM}"}
        assert same(c["seen"]["observation.state"], sh) and same(c["seen"][f"observation.images.{CAM}"], ih[0]), t
        if t == RESET_AT:
            frame = imgprep.prep_reference(c["image"], lut, None, [(x0, y0, 0)] * N, CROP)
            for e in RESET_ENVS:
                assert c["elapsed"][e] == 0
                for k in range(K):
                    assert same(c["seen"][f"observation.images.{CAM}"][e, k], frame[e]), (e, k)
                assert same(c["seen"]["observation.state"][e, 0], c["seen"]["observation.state"][e, 1])
            other = [e for e in range(N) if e not in RESET_ENVS]
            assert not np.array_equal(c["seen"]["observation.state"][other, 0], c["seen"]["observation.state"][other, 1])
    return ran


def check_run(records, calls):
    assert len(records) == EPISODES and all(r["length"] == STEPS for r in records)
    assert len(calls) > RESET_AT and calls[RESET_AT]["seen"] is not None
    assert any(len(set(c["elapsed"].tolist())) > 1 for c in calls), "the envs' episodes never ran out of phase"


def test_ensemble_mode_sees_the_history_of_every_call(venv):
    history, records, calls = evaluate(venv, ensemble=0.01)
    check_run(records, calls)
    assert replay(history, calls) == len(calls)


def test_queue_mode_skips_the_policy_not_the_history(venv):
    history, records, calls = evaluate(venv, n_action_steps=3, predict="when_needed")
    check_run(records, calls)
    ran = replay(history, calls)
    assert 0 < ran < len(calls)


def test_without_observe_the_policy_reads_the_envs_observation(venv):
    seen = []

    def predict_chunk(obs, info):
        seen.append(obs)
        return torch.zeros((N, C, venv.nj), dtype=torch.float32, device=venv.device)
    select, executor = chunked_policy(venv, predict_chunk, C, ensemble=0.01)
    obs, info = venv.reset(seed=1)
    select(obs, info)
    assert seen[0] is obs


# ---- training --------------------------------------------------------------------------------------------------------------------------
CAMS = {"cam_a": (16, 24), "cam_b": (24, 32)}
LENS = (2, 9)
TCROP = (12, 20)
KT = 3


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """The episode files, the data set on the device and the specification's view of it (computed once, shared, never changed)."""
    root = tmp_path_factory.mktemp("tiny_hist")
    rng = np.random.default_rng(25)
    paths, frames, state, action = [], {c: [] for c in CAMS}, [], []
    for e, T in enumerate(LENS):
        ep = {"/observations/qpos": rng.standard_normal((T, 21)).astype(np.float32), "/action": rng.standard_normal((T, 21)).astype(np.float32)}
        for c, (H, W) in CAMS.items():
            ep[f"/observations/images/{c}"] = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
        paths.append(harness.save_episode(ep, str(root), e, jpeg_quality=90))
        for c, ss in harness.episode_streams(harness.load_episode(paths[-1])).items():
            frames[c] += [jpeg.decode_reference(s) for s in ss]
        state.append(ep["/observations/qpos"])
        action.append(ep["/action"])
    ds = dataset.CompressedDataset(paths, list(CAMS))
    ref = {"frames": {c: np.stack(v) for c, v in frames.items()}, "state": np.concatenate(state), "action": np.concatenate(action),
           "episode": np.repeat(np.arange(len(LENS)), LENS), "frame": np.concatenate([np.arange(T) for T in LENS])}
    yield ds, ref, ds.stats()
    ds.close()


def assemble(ref, st, part, boxes, chunk, crop, K=None, aug=None):
    """The batch of the frames `part` in numpy; K None: as before n_obs_steps existed."""
    starts = np.concatenate([[0], np.cumsum(LENS)[:-1]])
    B = len(part)
    norm = lambda key, x: (x - st[key]["mean"]) / st[key]["std"]
    out = {"episode_index": ref["episode"][part], "frame_index": ref["frame"][part]}
    index, pad = imgprep.chunk_index(starts, LENS, part, chunk)
    out["action"], out["action_is_pad"] = norm("action", ref["action"][index]), pad
    if K is None:
        src, rep = part, lambda a: a
        out["observation.state"] = norm("observation.state", ref["state"][part])
    else:
        hidx, hpad = imgprep.history_index(starts, LENS, part, K)
        src, rep = hidx.reshape(-1), lambda a: np.repeat(a, K, axis=0)
        out["observation.state"] = norm("observation.state", ref["state"][hidx])
        out["observation.state_is_pad"] = hpad
    for ci, c in enumerate(CAMS):
        s = st[f"observation.images.{c}"]
        if aug is None:
            img = imgprep.prep_reference(ref["frames"][c][src], imgprep.normalise_lut(s["mean"], s["std"])[None], None, rep(boxes[c]), crop)
        else:
            mask, fac = aug[c]
            img = imgaug.jitter_reference(ref["frames"][c][src], imgaug.pack_params(rep(boxes[c]), rep(mask), rep(fac)), crop, s["mean"], s["std"])
        if K is not None:
            img = img.reshape(B, K, 3, *crop)
            out[f"observation.images.{c}_is_pad"] = hpad
        out[f"observation.images.{c}"] = img
    return out


def same_batch(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k].cpu().numpy()
        if w.dtype == np.float32:
            assert same(g, w), k
        else:
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


@pytest.mark.parametrize("augment", [None, True])
def test_history_batches_equal_their_numpy_assembly(data, augment):
    ds, ref, st = data
    tb = dataset.TrainingBatches(ds, batch_size=4, chunk_size=3, stats=st, crop=TCROP, crop_mode="center", seed=7, drop_last=False, n_obs_steps=KT, augment=augment)
    got, plan, aug = list(tb), tb.plan(0), tb.augment_plan(0)
    assert [int(g["frame_index"].shape[0]) for g in got] == [4, 4, 3] and (aug is None) == (augment is None)
    pads = 0
    for b, (g, (part, boxes)) in enumerate(zip(got, plan)):
        assert tuple(g["observation.images.cam_b"].shape) == (len(part), KT, 3) + TCROP and tuple(g["observation.state"].shape) == (len(part), KT, 21)
        same_batch(g, assemble(ref, st, part, boxes, 3, TCROP, K=KT, aug=None if aug is None else aug[b]))
        pads += int(g["observation.state_is_pad"].sum().item())
    assert pads == (2 + 1) + (2 + 1)          # the first two frames of both episodes
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 4, 3, st, n_obs_steps=0)


def test_without_n_obs_steps_the_batches_are_what_they_were(data):
    """the parent's output is its documented numpy assembly (tests/test_gpu_training_batches.py): same keys, same bits, same draws"""
    ds, ref, st = data
    for kw in (dict(), dict(n_obs_steps=None)):
        tb = dataset.TrainingBatches(ds, batch_size=4, chunk_size=3, stats=st, crop=TCROP, seed=7, **kw)
        for epoch in range(2):
            got = list(tb)
            plan = dataset.epoch_plan(11, 4, CAMS, TCROP, "random", seed=7, epoch=epoch)
            assert len(got) == len(plan) == 2
            for g, (part, boxes) in zip(got, plan):
                same_batch(g, assemble(ref, st, part, boxes, 3, TCROP))
    aug = dataset.TrainingBatches(ds, batch_size=4, chunk_size=3, stats=st, crop=TCROP, seed=7, augment=True)
    for b, (g, (part, boxes)) in enumerate(zip(list(aug), aug.plan(0))):
        same_batch(g, assemble(ref, st, part, boxes, 3, TCROP, aug=aug.augment_plan(0)[b]))


def test_training_and_evaluation_stack_alike(data):
    """the nine frames of episode 1, pushed in order through ObsHistory, are the batch entries of those frames"""
    ds, ref, st = data
    cam, (H, W) = "cam_a", CAMS["cam_a"]
    tb = dataset.TrainingBatches(ds, batch_size=9, chunk_size=1, stats=st, crop=TCROP, crop_mode="center", n_obs_steps=KT)
    part = np.arange(LENS[0], LENS[0] + LENS[1])
    x0, y0 = imgprep.center_box((H, W), TCROP)
    batch = tb.make(part, {c: np.tile(np.array([[*imgprep.center_box(CAMS[c], TCROP), 0]], dtype=np.int32), (len(part), 1)) for c in CAMS})
    want_s, want_i = batch["observation.state"].cpu().numpy(), batch[f"observation.images.{cam}"].cpu().numpy()
    env = make_vec(PEG, 1, 10, cameras=[])
    try:
        hist = oh.ObsHistory(env, KT, stats=st, crop=TCROP, cameras=[cam], state_dim=21, fmt="gym", size=(H, W))
        frames = torch.from_numpy(ref["frames"][cam][part]).to(env.device)
        state = torch.from_numpy(ref["state"][part]).to(env.device)
        for t in range(len(part)):
            info = {"episode_id": torch.ones(1, dtype=torch.int64, device=env.device), "elapsed_steps": torch.full((1,), t, dtype=torch.int32, device=env.device)}
            out = hist.push({"observation.state": state[t:t + 1], f"observation.images.{cam}": frames[t:t + 1]}, info)
            assert same(out["observation.state"].cpu().numpy()[0], want_s[t]) and same(out[f"observation.images.{cam}"].cpu().numpy()[0], want_i[t]), t
    finally:
        env.close()
