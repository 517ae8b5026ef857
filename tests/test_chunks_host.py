"""The specification of per-env chunk execution (av_aloha_amd/chunks.py: ensemble_tables, ChunkReference, check_setup) on the host: against
a literal restatement of LeRobot's list-shifting ACTTemporalEnsembler written here with torch on the CPU, against a collections.deque per env,
and the freshness, starvation and refusal rules one by one."""
import collections

import numpy as np
import pytest

from av_aloha_amd import chunks
from av_aloha_amd.chunks import ChunkReference, check_setup, ensemble_tables

SHAPES = [(1, 1), (2, 1), (3, 2), (5, 21), (100, 21)]
COEFFS = [0.01, 0.0, -0.5]


def predictions(calls, N, C, A, seed):
    """standard-normal chunks with some exact zeros"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((calls, N, C, A)).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = 0.0
    return x


class ListEnsembler:
    """LeRobot's ACTTemporalEnsembler.update for a batch of one, with the specification's tables: the first call clones; later calls scale
    the kept actions by cum[count - 1], add the new predictions times w[count], divide by cum[count], clamp the count, append the last
    prediction, and pop the first."""

    def __init__(self, C, tables):
        import torch
        self.torch, self.C = torch, C
        self.w, self.cum = torch.from_numpy(tables[0].copy()), torch.from_numpy(tables[1].copy())
        self.ens = None

    def update(self, y):
        torch = self.torch
        y = torch.from_numpy(np.ascontiguousarray(y))[None]          # [1, C, A]
        if self.ens is None:
            self.ens = y.clone()
            self.count = torch.ones((self.C, 1), dtype=torch.long)
        else:
            self.ens *= self.cum[self.count - 1]
            self.ens += y[:, :-1] * self.w[self.count]
            self.ens /= self.cum[self.count]
            self.count = torch.clamp(self.count + 1, max=self.C)
            self.ens = torch.cat([self.ens, y[:, -1:]], dim=1)
            self.count = torch.cat([self.count, torch.ones((1, 1), dtype=torch.long)])
        action, self.ens, self.count = self.ens[:, 0], self.ens[:, 1:], self.count[1:]
        return action[0].numpy().copy()


def test_ensemble_tables():
    for C in (1, 2, 100):
        for coeff in COEFFS:
            t = ensemble_tables(C, coeff)
            assert t.dtype == np.float32 and t.shape == (2, C)
            assert t[0, 0] == 1.0
            s, loop = np.float32(0), []
            for i in range(C):
                s = np.float32(s + t[0, i])
                loop.append(s)
            assert np.array_equal(t[1], np.array(loop, dtype=np.float32))
            assert np.array_equal(t[0], np.exp(np.float32(-coeff) * np.arange(C, dtype=np.float32)).astype(np.float32))


@pytest.mark.parametrize("coeff", COEFFS)
@pytest.mark.parametrize("C,A", SHAPES)
def test_ensemble_equals_the_list_shifting_algorithm(C, A, coeff):
    calls = 2 * C + 3
    tables = ensemble_tables(C, coeff)
    x = predictions(calls, 1, C, A, seed=C * 100 + A)
    ref = ChunkReference(1, C, A, "ensemble", tables=tables)
    lst = ListEnsembler(C, tables)
    for t in range(calls):
        a = ref.step(x[t], [0], [t])
        b = lst.update(x[t, 0])
        assert a.dtype == np.float32 and a.shape == (1, A)
        assert not np.isnan(a).any() and not np.isnan(b).any()
        assert np.array_equal(a[0], b), (C, A, coeff, t)


def test_coefficient_zero_is_the_running_mean():
    C, A, calls = 5, 3, 13
    x = predictions(calls, 1, C, A, seed=7).astype(np.float64)
    ref = ChunkReference(1, C, A, "ensemble", tables=ensemble_tables(C, 0.0))
    for t in range(calls):
        a = ref.step(x[t].astype(np.float32), [3], [t])
        made = [x[s, 0, t - s] for s in range(max(0, t - C + 1), t + 1)]          # the predictions made for time step t
        assert np.abs(a[0] - np.mean(made, axis=0)).max() <= 1e-6 * np.abs(made).max(), t          # relative to the predictions averaged


def test_unnormalise_is_a_multiplication_then_an_addition():
    C, A = 3, 4
    rng = np.random.default_rng(0)
    mean, std = rng.standard_normal(A).astype(np.float32), (rng.random(A) + 0.5).astype(np.float32)
    x = predictions(1, 2, C, A, seed=1)[0]
    q = ChunkReference(2, C, A, "queue", n_action_steps=C, mean=mean, std=std)
    a = q.step(x, [0, 1], [0, 0])
    want = (x[:, 0] * std).astype(np.float32) + mean
    assert np.array_equal(a, want.astype(np.float32))
    e = ChunkReference(2, C, A, "ensemble", tables=ensemble_tables(C, 0.01), mean=mean, std=std)
    assert np.array_equal(e.step(x, [0, 1], [0, 0]), want.astype(np.float32))


@pytest.mark.parametrize("C,k,f", [(1, 1, 0), (4, 4, 0), (4, 1, 0), (5, 2, 1), (16, 8, 1)])
def test_queue_equals_a_deque_per_env(C, k, f):
    N, A, calls = 4, 3, 3 * k + 5
    x = predictions(calls, N, C, A, seed=C + k)
    ref = ChunkReference(N, C, A, "queue", n_action_steps=k, first=f)
    queues = [collections.deque() for _ in range(N)]
    # env e's episodes last 3 + e steps: the envs' queues run empty in different calls
    elapsed, ids = np.zeros(N, dtype=np.int32), np.arange(N, dtype=np.int64)
    for t in range(calls):
        need = ref.need(ids, elapsed)
        for e in range(N):
            if elapsed[e] == 0:
                queues[e].clear()
            assert need[e] == (len(queues[e]) == 0)
            if not queues[e]:
                queues[e].extend(x[t, e, f:f + k])
        a = ref.step(x[t], ids, elapsed)
        for e in range(N):
            assert np.array_equal(a[e], queues[e].popleft()), (t, e)
        elapsed += 1
        over = elapsed > 2 + np.arange(N)
        ids[over] += N
        elapsed[over] = 0
    assert ref.starved == 0


def _ensemble_restarts(ref, C, A, x, ids, elapsed, env):
    """does the call return x's own row 0 for `env` -- what a fresh env returns, and (with distinct predictions) only a fresh one"""
    a = ref.step(x, ids, elapsed)
    return bool(np.array_equal(a[env], x[env, 0]))


def test_freshness_rules_one_at_a_time_and_together():
    N, C, A = 3, 4, 2
    x = predictions(8, N, C, A, seed=3)
    x[x == 0] = 0.5                                        # distinct predictions: an ensembled value is not a raw one
    tables = ensemble_tables(C, 0.01)
    ref = ChunkReference(N, C, A, "ensemble", tables=tables)
    ids = np.array([0, 1, 2], dtype=np.int64)
    # not stepped since set-up: fresh whatever id and elapsed say
    a = ref.step(x[0], ids, [5, 5, 5])
    assert np.array_equal(a, x[0][:, 0])
    # nothing changes: not fresh
    assert not _ensemble_restarts(ref, C, A, x[1], ids, [6, 6, 6], 0)
    # elapsed == 0 alone (the id stays: evaluate_vec restarts the ids at 0)
    a = ref.step(x[2], ids, [7, 0, 7])
    assert np.array_equal(a[1], x[2][1, 0]) and not np.array_equal(a[0], x[2][0, 0]) and not np.array_equal(a[2], x[2][2, 0])
    # an id change alone (a masked reset elsewhere keeps elapsed > 0 here)
    ids2 = np.array([0, 1, 9], dtype=np.int64)
    a = ref.step(x[3], ids2, [8, 1, 8])
    assert np.array_equal(a[2], x[3][2, 0]) and not np.array_equal(a[0], x[3][0, 0]) and not np.array_equal(a[1], x[3][1, 0])
    # both together
    ids3 = np.array([4, 1, 9], dtype=np.int64)
    a = ref.step(x[4], ids3, [0, 2, 9])
    assert np.array_equal(a[0], x[4][0, 0]) and not np.array_equal(a[1], x[4][1, 0]) and not np.array_equal(a[2], x[4][2, 0])
    # reset(): all envs unstepped
    ref.reset()
    assert np.array_equal(ref.step(x[5], ids3, [1, 3, 10]), x[5][:, 0])
    # the same three rules decide need() in queue mode
    q = ChunkReference(N, C, A, "queue", n_action_steps=4)
    assert q.need(ids, [5, 5, 5]).all()
    q.step(x[0], ids, [5, 5, 5])
    assert not q.need(ids, [6, 6, 6]).any()
    assert list(q.need(ids, [6, 0, 6])) == [False, True, False]
    assert list(q.need(ids2, [6, 6, 6])) == [False, False, True]
    assert list(q.need(ids3, [0, 6, 6])) == [True, False, True]
    q.reset()
    assert q.need(ids, [6, 6, 6]).all()
    # ... and need() changed nothing
    assert np.array_equal(q.step(x[1], ids, [6, 6, 6]), x[1][:, 0])


def test_starvation_repeats_the_previous_action_and_counts():
    N, C, A, k = 3, 4, 2, 2
    x = predictions(6, N, C, A, seed=5)
    ref = ChunkReference(N, C, A, "queue", n_action_steps=k)
    ids = np.array([0, 1, 2], dtype=np.int64)
    # fresh and starved: zeros
    a = ref.step(None, ids, [0, 0, 0])
    assert np.array_equal(a, np.zeros((N, A), np.float32)) and ref.starved == 3
    # starved again, no longer fresh: the previous action (zeros)
    a = ref.step(None, ids, [1, 1, 1])
    assert np.array_equal(a, np.zeros((N, A), np.float32)) and ref.starved == 6
    a0 = ref.step(x[0], ids, [2, 2, 2])
    assert np.array_equal(a0, x[0][:, 0])
    a1 = ref.step(None, ids, [3, 3, 3])                    # nobody needs: the queue's second row, nobody starves
    assert np.array_equal(a1, x[0][:, 1]) and ref.starved == 6
    a2 = ref.step(None, ids, [4, 4, 4])                    # the queues are empty: the previous action again
    assert np.array_equal(a2, a1) and ref.starved == 9
    # env 1 starts an episode while starved: zeros for it, the previous action for the others; the queues stay empty
    a3 = ref.step(None, np.array([0, 7, 2]), [5, 0, 5])
    assert np.array_equal(a3[0], a1[0]) and np.array_equal(a3[2], a1[2]) and np.array_equal(a3[1], np.zeros(A, np.float32)) and ref.starved == 12
    assert ref.need(np.array([0, 7, 2]), [6, 1, 6]).all()
    a4 = ref.step(x[1], np.array([0, 7, 2]), [6, 1, 6])
    assert np.array_equal(a4, x[1][:, 0])
    # ensemble mode has no starved calls: a chunk is required
    e = ChunkReference(N, C, A, "ensemble", tables=ensemble_tables(C, 0.01))
    with pytest.raises(ValueError):
        e.step(None, ids, [0, 0, 0])


def refusals(C=4, A=3):
    """(name, keyword arguments of check_setup) of every refusal of avsim_chunk_setup"""
    t = ensemble_tables(C, 0.01)

    def bad(i, j, v):
        b = t.copy()
        b[i, j] = v
        return b
    ok_q = dict(C=C, A=A, mode="queue", n_action_steps=2, first=1)
    ok_e = dict(C=C, A=A, mode="ensemble", tables=t)
    return [
        ("C = 0", {**ok_q, "C": 0}), ("C = 1025", {**ok_q, "C": 1025}), ("A = 0", {**ok_q, "A": 0}), ("A = 65", {**ok_q, "A": 65}),
        ("mode 2", {**ok_q, "mode": 2}), ("mode -1", {**ok_q, "mode": -1}),
        ("k = 0", {**ok_q, "n_action_steps": 0}), ("first < 0", {**ok_q, "first": -1}), ("first + k > C", {**ok_q, "n_action_steps": 3, "first": 2}),
        ("no tables", {**ok_e, "tables": None}), ("w nan", {**ok_e, "tables": bad(0, 1, np.nan)}), ("w inf", {**ok_e, "tables": bad(0, 2, np.inf)}),
        ("cum inf", {**ok_e, "tables": bad(1, 3, np.inf)}), ("cum 0", {**ok_e, "tables": bad(1, 0, 0.0)}), ("cum < 0", {**ok_e, "tables": bad(1, 2, -1.0)}),
        ("mean nan", {**ok_q, "mean": [0, np.nan, 0], "std": [1, 1, 1]}), ("std inf", {**ok_e, "mean": [0, 0, 0], "std": [1, np.inf, 1]}),
    ]


@pytest.mark.parametrize("name,kw", refusals(), ids=[r[0] for r in refusals()])
def test_check_setup_refuses(name, kw):
    with pytest.raises(ValueError):
        check_setup(**kw)


def test_check_setup_accepts_the_limits():
    assert check_setup(1, 1, "queue", n_action_steps=1)[:3] == (1, 1, 0)
    assert check_setup(1024, 64, "queue", n_action_steps=1024, first=0)[:3] == (1, 1024, 0)
    assert check_setup(1024, 64, "ensemble", tables=ensemble_tables(1024, 0.01))[0] == 0
    assert check_setup(4, 2, 1, n_action_steps=3, first=1)[:3] == (1, 3, 1)
    assert chunks.MODES == {"ensemble": 0, "queue": 1}
