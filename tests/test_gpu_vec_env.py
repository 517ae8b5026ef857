"""The device-resident vector env (av_aloha_amd/vec_env.py, avsim_episode_*, avsim_render_rgb_f32) against the host-pointer facade:
initial poses, reset state, NEXT_STEP autoreset, partial resets, divergence, evaluate_vec, policy-ready images, no synchronisation."""
import time

import numpy as np
import pytest

from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import VecEnv, make_vec, sample_poses
from avsim_test_util import host_observe
from gpu_util import torch as T

pytestmark = pytest.mark.gpu

TASKS = ("insert_peg", "slot_insertion", "sew_needle", "tube_transfer", "hook_package")
PEG = "gym_guided_vision/InsertPeg-3Arms-v0"


def dev_state(env):
    """qpos, qvel, ctrl, warm, latch, reset poses of a device-mode handle, as numpy."""
    h, N, d = env.h, env.num_envs, env.device
    q, v = T.empty((N, h.nq), dtype=T.float64, device=d), T.empty((N, h.nv), dtype=T.float64, device=d)
    c, w = T.empty((N, h.nu), dtype=T.float64, device=d), T.empty((N, h.nv), dtype=T.float64, device=d)
    lt, rp = T.empty(N, dtype=T.int32, device=d), T.empty((N, h.nobj, 7), dtype=T.float64, device=d)
    h.check(h.L.avsim_get_state(h.h, q.data_ptr(), v.data_ptr(), c.data_ptr(), w.data_ptr()))
    h.check(h.L.avsim_get_latch(h.h, lt.data_ptr()))
    h.check(h.L.avsim_get_reset_poses(h.h, rp.data_ptr()))
    return [x.cpu().numpy() for x in (q, v, c, w, lt, rp)]


def host_twin(task, poses, f64=False):
    sim = BatchedSim(task, 3, len(poses), f64=f64)
    sim.reset(poses)
    return sim


def home_action(env):
    return env._ap.float().clone()


@pytest.mark.parametrize("arms", [3, 2])
def test_sample_poses_equal_the_numpy_restatement(arms):
    ids = np.random.default_rng(5).integers(0, 2 ** 62, 1000)
    ids[:3] = [0, 1, 2 ** 40 + 3]
    for task in TASKS:
        env = VecEnv(task, arms, 2, 10, cameras=())
        for seed in (0, 2 ** 33 + 17):
            got, want = env.sample_poses(ids, seed=seed), sample_poses(task, seed, ids)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (task, arms, seed, bad[:4].tolist(), got[tuple(bad[0])].hex(), want[tuple(bad[0])].hex())
        env.close()


@pytest.mark.parametrize("task", ["slot_insertion", "tube_transfer"])
def test_reset_state_equals_the_host_reset(task):
    env = VecEnv(task, 3, 4, 10, cameras=())
    obs, info = env.reset(seed=5)
    ids = info["episode_id"].cpu().numpy()
    assert ids.tolist() == [0, 1, 2, 3]
    sim = host_twin(task, sample_poses(task, 5, ids))
    got = dev_state(env)
    want = list(sim.get_state()) + [sim.get_latch(), sim.get_reset_poses()]
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.array_equal(obs["observation.state"].cpu().numpy(), host_observe(sim).astype(np.float32))
    assert np.array_equal(env._ap.cpu().numpy(), host_observe(sim))
    env.close(); sim.close()


def test_next_step_autoreset():
    runs = []
    for variant in range(2):
        env = make_vec(PEG, 2, 5, cameras=[], obs_format="gym")
        obs, info = env.reset(seed=1)
        a = home_action(env)
        a[:, 0] += 0.05
        out = []
        for t in range(1, 10):
            act = a.clone()
            if t == 6:
                act[:, 1] += 0.3 * (variant + 1)          # the action of the reset step never reaches the new episode
            obs, r, te, tr, info = env.step(act)
            out.append([x.cpu().numpy().copy() for x in (obs["agent_pos"], r, te, tr, info["episode_id"], info["elapsed_steps"], info["is_success"])])
            if t == 5:
                assert tr.all() and (info["elapsed_steps"] == 5).all()
            if t == 6:
                assert (r == 0).all() and not te.any() and not tr.any() and not info["is_success"].any()
                assert info["episode_id"].tolist() == [2, 3] and (info["elapsed_steps"] == 0).all()
                sim = host_twin("insert_peg", sample_poses("insert_peg", 1, [2, 3]))
                assert np.array_equal(obs["agent_pos"].cpu().numpy(), host_observe(sim))
                sim.close()
        runs.append(out)
        env.close()
    for t in range(9):
        for k in range(7):
            assert np.array_equal(runs[0][t][k], runs[1][t][k]), (t, k)


@pytest.mark.parametrize("f64", [False, True])
def test_staggered_partial_resets_match_host_episodes(f64):
    """Partial resets (reset_mask) between steps and NEXT_STEP autoresets: every env's per-step agent_pos, reward and success equal a
    host BatchedSim stepped through the same episode from the same poses, bit for bit."""
    task, N, steps = "slot_insertion", 3, 16
    env = VecEnv(task, 3, N, 6, cameras=(), f64=f64)
    obs, info = env.reset(seed=11)
    rng = np.random.default_rng(0)
    base = env._ap.cpu().numpy().astype(np.float32)
    hosts = [None] * N

    def start(i, eid, ap):
        if hosts[i] is not None:
            hosts[i].close()
        hosts[i] = host_twin(task, sample_poses(task, 11, [eid]), f64=f64)
        assert np.array_equal(ap[i], host_observe(hosts[i])[0])

    ids = info["episode_id"].cpu().numpy()
    for i in range(N):
        start(i, ids[i], env._ap.cpu().numpy())
    for t in range(steps):
        if t in (4, 9):
            mask = np.array([t == 4, t == 9, t == 9])
            obs, info = env.reset(options={"reset_mask": T.as_tensor(mask)})
            ap, nid = env._ap.cpu().numpy(), info["episode_id"].cpu().numpy()
            for i in range(N):
                if mask[i]:
                    assert nid[i] > ids[i]
                    start(i, nid[i], ap)
                else:
                    assert nid[i] == ids[i]
            ids = nid
        a = (base + rng.normal(0, 0.05, base.shape)).astype(np.float32)
        obs, r, te, tr, info = env.step(T.as_tensor(a, device=env.device))
        ap, rw, su = env._ap.cpu().numpy(), r.cpu().numpy(), info["is_success"].cpu().numpy()
        el, nid = info["elapsed_steps"].cpu().numpy(), info["episode_id"].cpu().numpy()
        for i in range(N):
            if el[i] == 0:
                assert rw[i] == 0 and nid[i] > ids[i]
                start(i, nid[i], ap)
            else:
                hap, hrw, hsu = hosts[i].step(a[i:i + 1])
                assert np.array_equal(ap[i], hap[0]) and rw[i] == hrw[0] and bool(su[i]) == bool(hsu[0]), (t, i)
        ids = nid
    env.close()
    for s in hosts:
        s.close()


def test_divergence_truncates_and_restarts_only_that_env():
    runs = []
    for poke in (False, True):
        env = make_vec("gym_guided_vision/SlotInsertion-3Arms-v0", 3, 50, cameras=[], obs_format="gym")
        env.reset(seed=3)
        a = home_action(env)
        rows = []
        for t in range(6):
            if poke and t == 2:
                h = env.h
                v = T.empty((3, h.nv), dtype=T.float64, device=env.device)
                h.check(h.L.avsim_get_state(h.h, None, v.data_ptr(), None, None))
                v[1, 30] = 1e9
                h.check(h.L.avsim_set_state(h.h, None, v.data_ptr(), None, None))
            obs, r, te, tr, info = env.step(a)
            rows.append([x.cpu().numpy().copy() for x in (obs["agent_pos"], r, tr, info["episode_id"], info["elapsed_steps"], info["diverged"])])
            if poke and t == 2:
                assert tr.tolist() == [False, True, False] and info["diverged"].tolist() == [False, True, False]
            if poke and t == 3:
                assert info["elapsed_steps"].tolist() == [4, 0, 4] and info["episode_id"].tolist() == [0, 3, 2]
                assert not info["diverged"].any()
        runs.append(rows)
        env.close()
    for t in range(6):
        for k in range(6):
            assert np.array_equal(runs[0][t][k][[0, 2]], runs[1][t][k][[0, 2]]), (t, k)


def test_evaluate_vec_records_do_not_depend_on_the_batch():
    from av_aloha_amd.harness import evaluate_vec

    def policy(obs, info):
        s = obs["observation.state"]
        ph = 0.5 * info["elapsed_steps"].to(T.float32) + info["episode_id"].to(T.float32)
        a = s.clone()
        a[:, :6] += 0.05 * T.sin(ph)[:, None]
        return a

    recs = []
    for N in (3, 4, 10):
        env = make_vec(PEG, N, 6, cameras=[], seed=9)
        recs.append(evaluate_vec(env, policy, 12))
        env.close()
    for r in recs:
        assert [x["episode_id"] for x in r] == list(range(12)) and all(x["length"] == 6 for x in r)
    for r in recs[1:]:
        for x, y in zip(recs[0], r):
            assert x["return"] == y["return"] and x["max_reward"] == y["max_reward"] and x["success"] == y["success"]
            assert np.array_equal(x["initial_object_poses"], y["initial_object_poses"])
    assert np.array_equal(recs[0][5]["initial_object_poses"], sample_poses("insert_peg", 9, [5])[0])


def test_lerobot_images_are_preprocessed_gym_images():
    from av_aloha_amd.env import make
    from av_aloha_amd.harness import preprocess_observation
    cams = ["zed_cam_left", "wrist_cam_right"]
    le = make_vec(PEG, 2, 20, cameras=cams, obs_format="lerobot", seed=4)
    gy = make_vec(PEG, 2, 20, cameras=cams, obs_format="gym", seed=4)
    host = make(PEG, cameras=cams, num_envs=2)
    ol, _ = le.reset()
    og, _ = gy.reset()
    host.sim.reset(sample_poses("insert_peg", 4, [0, 1]))
    host._refresh_agent_pos()
    ho = host.get_obs()
    for c in cams:
        assert np.array_equal(og["pixels"][c].cpu().numpy(), ho["pixels"][c])
    a = home_action(gy)
    a[:, 2] += 0.1
    for step in range(2):
        g = {"pixels": {c: og["pixels"][c].cpu().numpy() for c in cams}, "agent_pos": og["agent_pos"].cpu().numpy()}
        pre = preprocess_observation(g)
        for c in cams:
            k = f"observation.images.{c}"
            assert ol[k].is_contiguous() and tuple(ol[k].shape) == (2, 3, 480, 640)
            assert T.equal(ol[k].cpu(), pre[k]), (step, c)
        assert T.equal(ol["observation.state"].cpu(), pre["observation.state"])
        ol, *_ = le.step(a)
        og, *_ = gy.step(a)
    assert le.check_render_overflow() == 0
    le.close(); gy.close(); host.close()


def test_step_does_not_synchronise():
    env = make_vec(PEG, 4, 20, cameras=["zed_cam_left"], obs_format="lerobot", observation_height=96, observation_width=128)
    env.reset(seed=0)
    a = home_action(env)
    env.step(a)
    T.cuda.synchronize()
    s = T.cuda.current_stream()
    t0 = time.perf_counter()
    T.cuda._sleep(int(2e9))            # about a second of GPU time in front of the step
    env.step(a)
    busy = not s.query()
    dt = time.perf_counter() - t0
    T.cuda.synchronize()
    assert busy and dt < 0.3, (busy, dt)
    env.close()
