"""Host model of the vector env's episode bookkeeping (avsim_episode_*): plain numpy, no GPU, no torch.

It restates the documented semantics (include/avsim.h, "Per-env episodes on the device"; the header comment of k_episode), not the
kernel's code: there is no ballot, no scan and no chunk here, only "the envs that start an episode in a call take the next ids of the
counter in env-index order".

    m = EpisodeModel("slot_insertion", N, seed, max_steps, term_on_success, log_cap)       # = avsim_episode_setup
    out = m.reset(mask)                   # = avsim_episode_reset: {"start", "id"}
    out = m.step(rw, su, diverged)        # = avsim_episode_step's bookkeeping on the physics launch's reward / success / diag bit 0
    m.log(n)                              # = avsim_episode_log

Every call also appends to m.events (one entry per call: kind, the starting envs, their ids, the envs that ended and why), which is
what the invariant and coverage checks read."""
import numpy as np

from av_aloha_amd.vec_env import OBJECT_BOXES, sample_poses


class EpisodeModel:
    def __init__(self, task, num_envs, seed, max_steps, term_on_success=False, log_cap=0):
        N = int(num_envs)
        self.task, self.N, self.seed = task, N, int(seed)
        self.max_steps, self.term_on_success, self.log_cap = int(max_steps), bool(term_on_success), int(log_cap)
        self.nobj = len(OBJECT_BOXES[task][1])
        # per env: no episode yet, every env starts one at its next reset / step
        self.id = np.full(N, -1, dtype=np.int64)
        self.elapsed = np.zeros(N, dtype=np.int32)
        self.ret = np.zeros(N)
        self.maxr = np.zeros(N, dtype=np.int32)
        self.succ = np.zeros(N, dtype=bool)
        self.pending = np.ones(N, dtype=bool)
        self.obj0 = np.zeros((N, self.nobj, 7))          # the running episode's sampled initial poses
        # global
        self.started = 0
        self.finished = 0
        L = self.log_cap
        self.log_ret, self.log_len = np.zeros(L), np.zeros(L, dtype=np.int32)
        self.log_maxr, self.log_succ = np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.uint8)
        self.log_obj = np.zeros((L, self.nobj, 7))
        self.events = []

    def _start(self, start):
        """The envs of `start` begin episodes: ids started + rank in env-index order; fresh per-env state."""
        idx = np.flatnonzero(start)
        ids = self.started + np.arange(len(idx), dtype=np.int64)
        self.started += len(idx)
        self.id[idx] = ids
        self.elapsed[idx] = 0
        self.ret[idx] = 0.0
        self.maxr[idx] = 0
        self.succ[idx] = False
        self.pending[idx] = False
        if len(idx):
            self.obj0[idx] = sample_poses(self.task, self.seed, ids)
        return idx, ids

    def poses(self):
        """[N, nobj, 7]: the initial poses of every env's running episode (zeros before its first)."""
        return self.obj0.copy()

    def reset(self, mask=None):
        start = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask).astype(bool).copy()
        assert start.shape == (self.N,)
        idx, ids = self._start(start)
        self.events.append({"kind": "reset", "start": idx, "ids": ids, "ended": np.zeros(0, dtype=np.int64)})
        return {"start": start, "id": self.id.copy()}

    def step(self, rw, su, diverged):
        rw, su, diverged = np.asarray(rw).astype(np.int32), np.asarray(su).astype(bool), np.asarray(diverged).astype(bool)
        assert rw.shape == su.shape == diverged.shape == (self.N,)
        start = self.pending.copy()
        book = ~start
        idx, ids = self._start(start)
        # the others book the step the launch took
        self.elapsed[book] += 1
        self.ret[book] += rw[book].astype(np.float64)
        self.maxr[book] = np.maximum(self.maxr[book], rw[book])
        self.succ[book] |= su[book]
        trunc = book & ((self.elapsed >= self.max_steps) | diverged)
        term = book & su if self.term_on_success else np.zeros(self.N, dtype=bool)
        end = term | trunc
        self.pending[end] = True
        self.finished += int(end.sum())
        e = np.flatnonzero(end)
        rec = e[self.id[e] < self.log_cap]
        k = self.id[rec]
        self.log_ret[k], self.log_len[k] = self.ret[rec], self.elapsed[rec]
        self.log_maxr[k], self.log_succ[k] = self.maxr[rec], self.succ[rec]
        self.log_obj[k] = self.obj0[rec]
        self.events.append({"kind": "step", "start": idx, "ids": ids, "ended": e, "ended_ids": self.id[e].copy(), "ended_len": self.elapsed[e].copy(),
                            "terminated": np.flatnonzero(term), "diverged": np.flatnonzero(book & diverged)})
        return {"start": start,
                "reward": np.where(start, 0, rw).astype(np.int32), "success": np.where(start, False, su),
                "terminated": term, "truncated": trunc, "id": self.id.copy(), "elapsed": self.elapsed.copy()}

    def count(self):
        return self.started, self.finished

    def log(self, n):
        assert 0 <= n <= self.log_cap
        return {"return": self.log_ret[:n].copy(), "length": self.log_len[:n].copy(), "max_reward": self.log_maxr[:n].copy(),
                "success": self.log_succ[:n].copy(), "obj_qpos0": self.log_obj[:n].copy()}


# ---- the scenario for a device test of this bookkeeping at batch scale: the part that needs no device -------------------------------

BOUNDARY = (0, 63, 64, 1023, 1024)        # both sides of the wave and the chunk boundary (and N - 1, added per batch size)
MAX_STEPS = 5
RESET_BEFORE = (3, 8)                     # masked resets before these step calls (1-based)
INSERT_BEFORE, POKE_BEFORE = 1, 6


def num_calls(N):
    """17 step calls.  An env starts an episode in a step call at most once per MAX_STEPS + 1 calls, so where the second wave or the
    second chunk is ONE env (N = 65: env 64, N = 1025: env 1024) that env cannot start in 5 of 17 step calls, which the coverage
    conditions ask of it.  Its timeline here is: masked reset before call 3, diverges in call 6, starts in calls 7, 13, 19, 25, 31 --
    so those two batch sizes run the same scenario for 31 calls (the first 17 are the same calls)."""
    return 31 if N in (65, 1025) else 17


def boundary_envs(N):
    return sorted({i for i in BOUNDARY + (N - 1,) if 0 <= i < N})


def scenario(N, seed):
    """The host-side choices of a run: reset masks (about 30 % of the envs; the boundary envs all in the first mask and in none of the
    second), the envs given the inserted state (about 10 %, the boundary envs among them), the two envs whose qvel is poked (boundary
    envs: mid-episode in call 6 because the first mask restarted them before call 3), and the per-call action noise seed."""
    rng = np.random.default_rng(seed)
    b = np.array(boundary_envs(N))
    masks = {}
    for k, call in enumerate(RESET_BEFORE):
        m = rng.random(N) < 0.3
        m[b] = k == 0
        masks[call] = m
    inserted = rng.random(N) < 0.1
    inserted[b] = True
    poke = sorted({63 if N > 63 else 0, N - 1})       # N >= 1025: one below and one at or above index 1024
    return {"masks": masks, "inserted": inserted, "poke": np.array(poke), "calls": num_calls(N), "action_seed": seed + 1}


def check_invariants(m):
    """The model's own invariants, from its event list and state (AssertionError names the one that fails)."""
    ids = np.concatenate([e["ids"] for e in m.events]) if m.events else np.zeros(0, dtype=np.int64)
    assert np.array_equal(np.sort(ids), np.arange(m.started)), "the ids handed out are not exactly range(started)"
    for c, e in enumerate(m.events):
        assert (np.diff(e["start"]) > 0).all() and (np.diff(e["ids"]) == 1).all(), f"call {c}: ids do not increase with the env index"
    assert m.finished == sum(len(e["ended"]) for e in m.events), "finished != number of end events"
    for e in m.events:
        if e["kind"] == "step":
            assert ((e["ended_len"] >= 1) & (e["ended_len"] <= m.max_steps)).all(), "an episode ended with a length outside [1, max_steps]"
    done = m.log_len > 0
    assert ((m.log_len[done] >= 1) & (m.log_len[done] <= m.max_steps)).all(), "a record's length is outside [1, max_steps]"
    # Every episode started has finished, is running, or was cut short by a reset of its env, which neither finishes nor records it.
    # The event list is replayed here on its own: an env's id is superseded only in a reset call unless it has ended, an episode ends
    # once and under the id its env holds, and what is left running is what the model's state says.  Without resets of running envs
    # this is "started - finished = the envs that hold an id and are not pending".
    cur = np.full(m.N, -1, dtype=np.int64)        # the id each env holds
    live = np.zeros(m.N, dtype=bool)              # ... and has not ended
    cut = 0
    for c, e in enumerate(m.events):
        over = live[e["start"]]
        assert e["kind"] == "reset" or not over.any(), f"call {c}: a step call restarted an env whose episode had not ended"
        cut += int(over.sum())
        cur[e["start"]], live[e["start"]] = e["ids"], True
        if e["kind"] == "step":
            assert live[e["ended"]].all() and np.array_equal(cur[e["ended"]], e["ended_ids"]), f"call {c}: an episode ended that was not running"
            assert not np.isin(e["ended"], e["start"]).any(), f"call {c}: an env started and ended in one call"
            live[e["ended"]] = False
    assert np.array_equal(cur, m.id) and np.array_equal(live, (m.id >= 0) & ~m.pending), "the model's ids / pending flags are not what its events say"
    assert m.started - m.finished - cut == int(live.sum()), "started - finished - cut short != envs that run an episode"


def coverage(m, N):
    """Figures of the coverage conditions that the model alone decides (step calls only)."""
    steps = [e for e in m.events if e["kind"] == "step"]

    def split_calls(width):
        n = 0
        for e in steps:
            inside = int((e["start"] < width).sum())
            n += 0 < inside < min(width, N) and inside < len(e["start"])
        return n
    ended = np.concatenate([e["ended_ids"] for e in steps]) if steps else np.zeros(0, dtype=np.int64)
    return {"wave_split_calls": split_calls(64), "chunk_split_calls": split_calls(1024),
            "terminated": sum(len(e["terminated"]) for e in steps), "diverged": sum(len(e["diverged"]) for e in steps),
            "ended_below_cap": int((ended < m.log_cap).sum()), "ended_at_or_above_cap": int((ended >= m.log_cap).sum())}
