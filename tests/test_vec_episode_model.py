"""The host model of the episode bookkeeping (tests/vec_episode_model.py) on synthetic streams: its invariants at three chunks of envs,
its records, and that the batch-scale scenario (masked resets, a divergence, 65 / 1025 / 2051 envs) reaches the regimes it is there for."""
import numpy as np
import pytest

from av_aloha_amd.vec_env import sample_poses
from vec_episode_model import MAX_STEPS, POKE_BEFORE, EpisodeModel, boundary_envs, check_invariants, coverage, scenario

TASK = "slot_insertion"


@pytest.mark.parametrize("tos", [False, True])
def test_invariants_on_random_streams(tos):
    """Random rewards, successes, divergences and reset masks at N = 2051 (three chunks of 1024): the ids handed out are range(started),
    each once and increasing with the env index inside a call; finished counts the end events; every length is in [1, max_steps];
    started - finished = the envs that run an episode.  Checked after every call."""
    N, cap = 2051, 3000
    rng = np.random.default_rng(21 + tos)
    m = EpisodeModel(TASK, N, 5, MAX_STEPS, tos, cap)
    ends = 0
    for call in range(40):
        if rng.random() < 0.2:
            m.reset(rng.random(N) < rng.choice([0.0, 0.01, 0.3, 1.0]))
        running = (m.id >= 0) & ~m.pending
        out = m.step(rng.integers(0, 5, N), rng.random(N) < 0.05, rng.random(N) < 0.01)
        ended = out["terminated"] | out["truncated"]
        assert not (ended & ~running).any() and not (out["terminated"] & ~np.bool_(tos)).any()
        assert (out["elapsed"][out["start"]] == 0).all() and (out["reward"][out["start"]] == 0).all()
        ends += int(ended.sum())
        check_invariants(m)
    assert m.count() == (m.started, ends) and ends > cap                  # ids on both sides of the cap finished
    log = m.log(cap)
    assert (log["length"] > 0).sum() > 0 and (log["length"] == 0).sum() > 0
    done = log["length"] > 0
    assert np.array_equal(log["obj_qpos0"][done], sample_poses(TASK, 5, np.flatnonzero(done)))
    assert not log["obj_qpos0"][~done].any() and not log["return"][~done].any()
    assert (log["max_reward"][done] <= 4).all() and (log["return"][done] <= 4.0 * log["length"][done]).all()
    if tos:          # a terminated episode's record has seen the success
        assert log["success"][done][log["length"][done] < MAX_STEPS].sum() > 0


def test_a_single_episode_by_hand():
    m = EpisodeModel(TASK, 2, 3, 3, True, 1)
    o = m.step([9, 9], [1, 1], [1, 1])             # the first call starts both: the launch's step is not booked
    assert o["id"].tolist() == [0, 1] and o["reward"].tolist() == [0, 0] and not o["success"].any() and not o["truncated"].any()
    o = m.step([1, 2], [0, 0], [0, 0])
    assert o["elapsed"].tolist() == [1, 1] and not (o["terminated"] | o["truncated"]).any()
    o = m.step([3, 4], [0, 1], [0, 0])
    assert o["terminated"].tolist() == [False, True] and o["truncated"].tolist() == [False, False] and m.count() == (2, 1)
    o = m.step([1, 7], [0, 1], [0, 0])             # env 0 reaches max_steps, env 1 starts id 2
    assert o["truncated"].tolist() == [True, False] and o["id"].tolist() == [0, 2] and o["elapsed"].tolist() == [3, 0]
    assert o["reward"].tolist() == [1, 0] and m.count() == (3, 2)
    o = m.reset([False, True])                     # env 0 stays pending, env 1 restarts
    assert o["id"].tolist() == [0, 3] and m.pending.tolist() == [True, False]
    o = m.step([0, 0], [0, 0], [0, 1])
    assert o["id"].tolist() == [4, 3] and o["truncated"].tolist() == [False, True] and m.count() == (5, 3)
    log = m.log(1)                                 # only id 0 is kept: ids 1 and 3 finished above the cap
    assert log["return"].tolist() == [5.0] and log["length"].tolist() == [3] and log["max_reward"].tolist() == [3] and log["success"].tolist() == [0]
    assert np.array_equal(log["obj_qpos0"], sample_poses(TASK, 3, [0]))
    check_invariants(m)


@pytest.mark.parametrize("N", [65, 1025, 2051])
def test_the_scenario_reaches_every_regime(N):
    """The batch-scale scenario on emulated physics (reward 0, no success; the poked envs diverge in call 6 and nothing else does): which
    envs start in which call is then decided by the masks, max_steps and the poke alone, as it is on the device without
    terminate_on_success.  In at least 5 step calls the starting set splits wave 0 and reaches past it, and for N >= 1025 splits chunk 0
    and reaches past it."""
    sc = scenario(N, 100 + N)
    b = boundary_envs(N)
    assert all(sc["masks"][3][i] and not sc["masks"][8][i] and sc["inserted"][i] for i in b)
    assert 0.2 < sc["masks"][3].mean() < 0.4 and 0.2 < sc["masks"][8].mean() < 0.4 and 0.05 < sc["inserted"].mean() < 0.15
    m = EpisodeModel(TASK, N, 11, MAX_STEPS, False, 0)
    m.reset()
    for call in range(1, sc["calls"] + 1):
        if call in sc["masks"]:
            m.reset(sc["masks"][call])
        div = np.zeros(N, dtype=bool)
        if call == POKE_BEFORE:
            div[sc["poke"]] = True
        m.step(np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool), div)
    check_invariants(m)
    m.log_cap = m.started // 2
    cov = coverage(m, N)
    assert cov["wave_split_calls"] >= 5, cov
    assert N < 1025 or cov["chunk_split_calls"] >= 5, cov
    assert cov["diverged"] == 2 and cov["terminated"] == 0, cov
    assert cov["ended_below_cap"] > 0 and cov["ended_at_or_above_cap"] > 0, cov
