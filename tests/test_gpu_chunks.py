"""Per-env chunk execution on the device (avsim_chunk_*, csrc/avsim_chunks.hip; chunks.ActionChunks, BatchedSim.chunk_*) against its
specification, av_aloha_amd.chunks.ChunkReference.  Every action of every call is compared by np.array_equal on float32 arrays with no NaN on
either side.  The handles are vector envs without cameras; no physics step is taken: episode ids and elapsed steps are tensors the tests
write.  Inputs: standard-normal chunks with some exact zeros, fixed seeds."""
import time

import numpy as np
import pytest

from av_aloha_amd import chunks as ck
from av_aloha_amd import images
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import make_vec
from avsim_test_util import same
from gpu_util import torch as T

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
SHAPES = [(1, 1), (2, 1), (3, 2), (5, 21), (100, 21), (7, 14)]
COEFFS = [0.01, 0.0, -0.5]


@pytest.fixture(scope="module")
def envs():
    """vector envs by size, made once and shared: the chunk state is re-initialised by every set-up"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = make_vec(PEG, N, 50, cameras=[])
        return made[N]
    yield get
    for e in made.values():
        e.close()


def predictions(calls, N, C, A, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((calls, N, C, A)).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = 0.0
    return x


def stats_for(A, seed=11):
    rng = np.random.default_rng(seed)
    return {"action": {"mean": rng.standard_normal(A).astype(np.float32), "std": (rng.random(A) + 0.25).astype(np.float32)}}


def info_of(env, ids, elapsed):
    return {"episode_id": T.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(env.device),
            "elapsed_steps": T.from_numpy(np.ascontiguousarray(elapsed, dtype=np.int32)).to(env.device)}


def run(env, ac, ref, x, ids, elapsed, give=None):
    """calls t = 0 .. len(x)-1 with ids[t], elapsed[t]; give[t] False: chunks=None.  Every action equal."""
    xd = T.from_numpy(x).to(env.device)
    for t in range(len(x)):
        g = give is None or give[t]
        a = ac.step(xd[t] if g else None, info_of(env, ids[t], elapsed[t])).cpu().numpy()
        b = ref.step(x[t] if g else None, ids[t], elapsed[t])
        assert same(a, b), (t, np.argwhere(a != b)[:4])


# ---- ensemble ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff", COEFFS)
@pytest.mark.parametrize("C,A", SHAPES)
def test_ensemble_equals_the_specification(envs, C, A, coeff):
    """2C + 3 calls: the ring wraps twice and the counts saturate; A = 21 and 14 put the rotation off 16-byte alignment on most calls.
    Env 2 starts anew once on the way (id change)."""
    N, calls = 3, 2 * C + 3
    env = envs(N)
    ids = np.tile(np.arange(N, dtype=np.int64), (calls, 1))
    ids[C + 2:, 2] += N
    elapsed = np.tile(np.arange(1, calls + 1, dtype=np.int32)[:, None], (1, N))
    for stats in (None, stats_for(A)):
        ac = ck.ActionChunks(env, C, A, ensemble=coeff, stats=stats)
        run(env, ac, ac.reference(), predictions(calls, N, C, A, seed=C * 64 + A), ids, elapsed)


def fresh_schedule(N, calls):
    """env e is made fresh on call (e mod 5) + 1, in the way (e // 5) mod 5 names: by id change only, by elapsed == 0 only, by both, twice
    on consecutive calls, never.  (Call 0 starts every env: none has been stepped.)"""
    ids = np.zeros((calls, N), dtype=np.int64)
    elapsed = np.zeros((calls, N), dtype=np.int32)
    cur_id, cur_el = np.arange(N, dtype=np.int64), np.ones(N, dtype=np.int32)
    e = np.arange(N)
    when, way = e % 5 + 1, (e // 5) % 5
    for t in range(calls):
        hit = when == t
        again = (when + 1 == t) & (way == 3)
        new_id = (hit & np.isin(way, (0, 2, 3))) | again
        zero = hit & np.isin(way, (1, 2))
        cur_id = np.where(new_id, cur_id + N, cur_id)
        cur_el = np.where(zero, 0, cur_el)
        ids[t], elapsed[t] = cur_id, cur_el
        cur_el = cur_el + 1
    return ids, elapsed


@pytest.mark.parametrize("N", [70, 1100])
def test_ensemble_large_batch_fresh_per_env(envs, N):
    """past one wave, and past one 1024-lane workgroup of the bookkeeping kernel"""
    C, A, calls = 4, 21, 9
    env = envs(N)
    ids, elapsed = fresh_schedule(N, calls)
    x = predictions(calls, N, C, A, seed=N)
    for coeff, stats in ((0.01, None), (-0.5, stats_for(A))) if N == 70 else ((0.01, stats_for(A)),):
        ac = ck.ActionChunks(env, C, A, ensemble=coeff, stats=stats)
        run(env, ac, ac.reference(), x, ids, elapsed)


# ---- queue -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,k,f", [(1, 1, 0), (4, 4, 0), (4, 1, 0), (5, 2, 1), (16, 8, 1)])
def test_queue_need_none_calls_and_starvation(envs, C, k, f):
    N, A, calls = 5, 21, 3 * k + 9
    env = envs(N)
    x = predictions(calls, N, C, A, seed=C * 8 + k)
    xd = T.from_numpy(x).to(env.device)
    for stats in (None, stats_for(A)):
        ac = ck.ActionChunks(env, C, A, n_action_steps=k, first=f, stats=stats)
        ref = ac.reference()
        ids, elapsed = np.arange(N, dtype=np.int64), np.zeros(N, dtype=np.int32)
        starve_on = {2, 3, calls - 2}
        for t in range(calls):
            info = info_of(env, ids, elapsed)
            need, flag = ac.need(info)
            want = ref.need(ids, elapsed)
            assert np.array_equal(need.cpu().numpy(), want) and int(flag.item()) == int(want.any()), t
            give = bool(want.any()) and t not in starve_on          # None where nobody needs; None on some calls where somebody does
            a = ac.step(xd[t] if give else None, info).cpu().numpy()
            b = ref.step(x[t] if give else None, ids, elapsed)
            assert same(a, b), t
            # env e's episodes last 2 + e steps (a new id, elapsed 0); env 4 changes id once WITHOUT elapsed 0
            elapsed += 1
            over = elapsed > 1 + np.arange(N)
            over[4] = False
            ids[over] += N
            elapsed[over] = 0
            if t == 5:
                ids[4] += N
        assert ref.starved > 0
        assert ac.starved() == ref.starved


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def raw_setup(env, C, A, mode, k, f, tables, ms):
    env._bind_stream()
    images.check_call(env.h, env.L.avsim_chunk_setup(env.h.h, C, A, mode, k, f, None if tables is None else tables.ctypes.data,
                                                     None if ms is None else ms.ctypes.data))


def test_refusals_leave_the_state_alone(envs):
    N, C, A = 3, 4, 3
    env = envs(N)
    t = ck.ensemble_tables(C, 0.01)

    def bad(i, j, v):
        b = t.copy()
        b[i, j] = v
        return b
    ms = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.float32)
    ms_nan, ms_inf = ms.copy(), ms.copy()
    ms_nan[0, 1], ms_inf[1, 2] = np.nan, np.inf
    refused = [(0, A, 1, 1, 0, None, None), (1025, A, 1, 1, 0, None, None), (C, 0, 1, 1, 0, None, None), (C, 65, 1, 1, 0, None, None),
               (C, A, 2, 1, 0, None, None), (C, A, -1, 1, 0, None, None), (C, A, 1, 0, 0, None, None), (C, A, 1, 1, -1, None, None), (C, A, 1, 3, 2, None, None),
               (C, A, 0, 0, 0, None, None), (C, A, 0, 0, 0, bad(0, 1, np.nan), None), (C, A, 0, 0, 0, bad(1, 3, np.inf), None), (C, A, 0, 0, 0, bad(1, 0, 0.0), None),
               (C, A, 0, 0, 0, bad(1, 2, -1.0), None), (C, A, 1, 2, 1, None, ms_nan), (C, A, 0, 0, 0, t, ms_inf)]
    calls = 3 + len(refused) + 2
    x = predictions(calls, N, C, A, seed=2)
    ids = np.tile(np.arange(N, dtype=np.int64), (calls, 1))
    elapsed = np.tile(np.arange(1, calls + 1, dtype=np.int32)[:, None], (1, N))
    ac = ck.ActionChunks(env, C, A, ensemble=0.01)
    ref = ac.reference()
    run(env, ac, ref, x[:3], ids[:3], elapsed[:3])
    for i, r in enumerate(refused):
        with pytest.raises(ValueError):
            raw_setup(env, *r)
        run(env, ac, ref, x[3 + i:4 + i], ids[3 + i:4 + i], elapsed[3 + i:4 + i])          # as if the refused call had not happened
    with pytest.raises(ValueError):                                                     # ensemble mode: a chunk in every call
        ac.step(None, info_of(env, ids[-2], elapsed[-2]))
    run(env, ac, ref, x[-2:], ids[-2:], elapsed[-2:])


def test_calls_before_the_setup_are_refused():
    env = make_vec(PEG, 2, 10, cameras=[])
    try:
        L, h = env.L, env.h.h
        info = info_of(env, [0, 1], [0, 0])
        a, n = T.zeros((2, 3), dtype=T.float32, device=env.device), T.zeros(2, dtype=T.uint8, device=env.device)
        c = np.zeros(1, dtype=np.uint64)
        for rc in (L.avsim_chunk_reset(h), L.avsim_chunk_need(h, info["episode_id"].data_ptr(), info["elapsed_steps"].data_ptr(), n.data_ptr(), None),
                   L.avsim_chunk_step(h, None, info["episode_id"].data_ptr(), info["elapsed_steps"].data_ptr(), a.data_ptr()),
                   L.avsim_chunk_starved(h, c.ctypes.data)):
            with pytest.raises(ValueError):
                images.check_call(env.h, rc)
    finally:
        env.close()


def test_a_second_setup_and_reset_start_over(envs):
    N, C, A = 3, 4, 2
    env = envs(N)
    x = predictions(6, N, C, A, seed=9)
    ids = np.tile(np.arange(N, dtype=np.int64), (6, 1))
    elapsed = np.tile(np.arange(1, 7, dtype=np.int32)[:, None], (1, N))
    ac = ck.ActionChunks(env, C, A, n_action_steps=2)
    ac.step(None, info_of(env, ids[0], elapsed[0]))
    assert ac.starved() == N
    ac = ck.ActionChunks(env, C, A, ensemble=0.0)
    assert ac.starved() == 0
    ref = ac.reference()
    run(env, ac, ref, x[:3], ids[:3], elapsed[:3])
    ac.reset()
    ref.reset()
    a = ac.step(T.from_numpy(x[3]).to(env.device), info_of(env, ids[3], elapsed[3])).cpu().numpy()
    assert same(a, x[3][:, 0]) and same(a, ref.step(x[3], ids[3], elapsed[3]))
    run(env, ac, ref, x[4:], ids[4:], elapsed[4:])


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_with_the_chunk_tensor_overwritten(envs):
    """twenty calls with no host wait in between; the one chunk tensor is overwritten as soon as each call has returned"""
    N, C, A, calls = 70, 4, 21, 20
    env = envs(N)
    ids, elapsed = fresh_schedule(N, calls)
    x = predictions(calls + 1, N, C, A, seed=4)
    xd = T.from_numpy(x).to(env.device)
    infos = [info_of(env, ids[t], elapsed[t]) for t in range(calls)]
    ac = ck.ActionChunks(env, C, A, ensemble=0.01, stats=stats_for(A))
    ref = ac.reference()
    buf, got = xd[0].clone(), []
    T.cuda.synchronize()
    for t in range(calls):
        got.append(ac.step(buf, infos[t]).clone())
        buf.copy_(xd[t + 1])
    T.cuda.synchronize()
    for t in range(calls):
        assert same(got[t].cpu().numpy(), ref.step(x[t], ids[t], elapsed[t])), t


@pytest.mark.parametrize("ensemble", [0.01, None])
def test_need_and_step_do_not_synchronise(envs, ensemble):
    N, C, A = 70, 4, 21
    env = envs(N)
    ac = ck.ActionChunks(env, C, A, ensemble=ensemble)
    x = T.from_numpy(predictions(1, N, C, A, seed=5)[0]).to(env.device)
    info = info_of(env, np.arange(N), np.ones(N))
    ac.need(info)
    ac.step(x, info)
    T.cuda.synchronize()
    s = T.cuda.current_stream()
    t0 = time.perf_counter()
    T.cuda._sleep(int(2e9))            # about a second of GPU time in front of the calls
    ac.need(info)
    ac.step(x, info)
    ac.reset()
    busy = not s.query()
    dt = time.perf_counter() - t0
    T.cuda.synchronize()
    assert busy and dt < 0.3, (busy, dt)


# ---- host I/O ------------------------------------------------------------------------------------------------------------------------
def test_batched_sim_ensemble_and_queue():
    N, C, A, calls = 5, 5, 21, 13
    sim = BatchedSim("insert_peg", 3, N)
    try:
        ids, elapsed = fresh_schedule(N, calls)
        x = predictions(calls, N, C, A, seed=6)
        st = stats_for(A)["action"]
        ref = ck.ChunkReference(N, C, A, **sim.chunk_setup(C, A, ensemble=0.01, mean=st["mean"], std=st["std"]))
        for t in range(calls):
            assert same(sim.chunk_step(x[t], ids[t], elapsed[t]), ref.step(x[t], ids[t], elapsed[t])), t
        with pytest.raises(ValueError):
            sim.chunk_step(None, ids[0], elapsed[0])
        ref = ck.ChunkReference(N, C, A, **sim.chunk_setup(C, A, n_action_steps=2, first=1))
        for t in range(calls):
            need, flag = sim.chunk_need(ids[t], elapsed[t])
            want = ref.need(ids[t], elapsed[t])
            assert np.array_equal(need, want) and flag == bool(want.any()), t
            give = bool(want.any()) and t != 4
            assert same(sim.chunk_step(x[t] if give else None, ids[t], elapsed[t]), ref.step(x[t] if give else None, ids[t], elapsed[t])), t
        assert sim.chunk_starved() == ref.starved
        with pytest.raises(ValueError):
            sim.chunk_setup(0, A)
    finally:
        sim.close()
