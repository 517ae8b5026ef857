"""What happens to a chunked policy's output before env.step: per-env execution of action chunks with LeRobot's exponential temporal
ensembling or an n-step action queue, un-normalisation and the episode-aware reset.

The numpy half of this module -- ensemble_tables, check_setup, ChunkReference -- is the SPECIFICATION: host only, float32 throughout,
every *, + and / rounded on its own (no fused multiply-add, no float64).  The device (avsim_chunk_*, csrc/avsim_chunks.hip) equals it bit
for bit.  ActionChunks is the device call on torch tensors for the owner of a device-I/O handle (vec_env.VecEnv);
sim.BatchedSim.chunk_setup / chunk_step / chunk_need are the same on numpy arrays.

A policy predicts a chunk [N, C, A] of NORMALISED actions (dataset.TrainingBatches(chunk_size=C) trains on (a - mean) / std); row k of env
i's chunk is its action for k steps from now.  LeRobot keeps one action queue or one temporal ensembler for the whole batch
(policy.reset() / policy.select_action()); here the state is per env, and an env that starts a new episode starts it with empty state.

Fresh: env i is fresh in a call when it has not been stepped since set-up or reset(), or elapsed[i] == 0, or episode_id[i] differs from the
id it had in the previous call.  (Both signals: harness.evaluate_vec restarts the ids at 0, so env 0 can go from id 0 to id 0; a masked
reset changes an id while the other envs keep elapsed > 0.)

Un-normalise first, as LeRobot does: y = x * std[a] + mean[a], two operations; without mean / std y = x.

Mode "ensemble" (ACTTemporalEnsembler, online): weights w[i] = exp(-coeff i), cum = cumsum(w); the oldest prediction of a time step has
weight w[0].  Per env u counts the updates since fresh, kept as a ring head u mod C and a count min(u, C - 1).  For k in 0 .. C-1:
c = min(u, C-1-k), slot j = (u + k) mod C, ens[j] = y[k] if c == 0 else (ens[j] * cum[c-1] + y[k] * w[c]) / cum[c].  The action is
ens[u mod C] after the update; then u += 1.  c is the count LeRobot carries in ensembled_actions_count, the ring replaces its cat / shift.

Mode "queue": n_action_steps = k >= 1 rows [first, first + k) of a chunk are executed one per call (ACT: first = 0; a diffusion policy:
first = n_obs_steps - 1).  An env NEEDS a chunk when it is fresh or its queue is empty.  step: an env that needs one takes y[first .. first+k)
from the given chunks; given none it is STARVED: it repeats its previous action (zeros if it is fresh), `starved` goes up by one and its
queue stays empty.  An env that does not need one ignores the given chunk.  Then the head of the queue is the action."""
from __future__ import annotations

import numpy as np

MODES = {"ensemble": 0, "queue": 1}
MAX_CHUNK, MAX_ACTION_DIM = 1024, 64


def ensemble_tables(C, coeff):
    """float32 [2, C]: w[i] = exp(float32(-coeff) * float32(i)) and its sequential float32 cumulative sum (ACT's default coeff: 0.01)."""
    w = np.exp(np.float32(-coeff) * np.arange(int(C), dtype=np.float32)).astype(np.float32)
    return np.stack([w, np.cumsum(w, dtype=np.float32)]).astype(np.float32)


def mean_std(mean, std, A):
    """None, or float32 [2, A] = (mean, std) for the library; both or neither."""
    if mean is None and std is None:
        return None
    if mean is None or std is None:
        raise ValueError("chunks: give both mean and std, or neither")
    ms = np.stack([np.asarray(mean, dtype=np.float32).reshape(-1), np.asarray(std, dtype=np.float32).reshape(-1)])
    if ms.shape != (2, int(A)):
        raise ValueError(f"chunks: mean / std have {ms.shape[1]} values, action_dim is {A}")
    return np.ascontiguousarray(ms)


def check_setup(C, A, mode, n_action_steps=None, first=0, tables=None, mean=None, std=None):
    """ValueError for what avsim_chunk_setup refuses -> (mode number, k, first, tables float32 [2, C] or None, mean_std float32 [2, A] or None)."""
    C, A = int(C), int(A)
    if not 1 <= C <= MAX_CHUNK:
        raise ValueError(f"chunks: chunk_size {C} outside 1..{MAX_CHUNK}")
    if not 1 <= A <= MAX_ACTION_DIM:
        raise ValueError(f"chunks: action_dim {A} outside 1..{MAX_ACTION_DIM}")
    if mode not in MODES and mode not in (0, 1):
        raise ValueError(f"chunks: mode {mode!r} ('ensemble' or 'queue')")
    m = MODES.get(mode, mode)
    k, f = 0, 0
    if m == 1:
        k, f = int(n_action_steps if n_action_steps is not None else 0), int(first)
        if k < 1 or f < 0 or f + k > C:
            raise ValueError(f"chunks: queue of n_action_steps {k} from row {f} of a chunk of {C} (k >= 1, first >= 0, first + k <= C)")
        tables = None
    else:
        if tables is None:
            raise ValueError("chunks: ensemble mode needs the tables (ensemble_tables)")
        tables = np.ascontiguousarray(tables, dtype=np.float32)
        if tables.shape != (2, C):
            raise ValueError(f"chunks: tables of shape {tables.shape}, expected (2, {C})")
        if not np.isfinite(tables).all():
            raise ValueError("chunks: a table entry that is not finite")
        if not (tables[1] > 0).all():
            raise ValueError("chunks: a cumulative weight that is not positive")
    ms = mean_std(mean, std, A)
    if ms is not None and not np.isfinite(ms).all():
        raise ValueError("chunks: a mean or std that is not finite")
    return m, k, f, tables, ms


class ChunkReference:
    """The specification as a state machine over N envs (the module's docstring).  need(episode_id, elapsed) -> bool [N] changes nothing
    (ensemble mode: every env needs a chunk in every call); step(chunks | None, episode_id, elapsed) -> float32 [N, A], a new array;
    reset(): all envs unstepped; starved: the count of starved env-calls since set-up."""

    def __init__(self, N, C, A, mode, tables=None, n_action_steps=None, first=0, mean=None, std=None):
        self.mode, self.k, self.first, tables, ms = check_setup(C, A, mode, n_action_steps, first, tables, mean, std)
        self.N, self.C, self.A = int(N), int(C), int(A)
        if self.N < 1:
            raise ValueError("chunks: N >= 1")
        self.w, self.cum = (tables[0].copy(), tables[1].copy()) if tables is not None else (None, None)
        self.mean, self.std = (ms[0].copy(), ms[1].copy()) if ms is not None else (None, None)
        self.starved = 0
        self.stepped = np.zeros(self.N, dtype=bool)
        self.last_id = np.zeros(self.N, dtype=np.int64)
        self.head = np.zeros(self.N, dtype=np.int64)          # ensemble: u mod C; queue: the next row of the queue
        self.count = np.zeros(self.N, dtype=np.int64)         # ensemble: min(u, C - 1); queue: the rows left
        self.buf = np.zeros((self.N, self.C if self.mode == 0 else self.k, self.A), dtype=np.float32)
        self.prev = np.zeros((self.N, self.A), dtype=np.float32)

    def reset(self):
        self.stepped[:] = False

    def _fresh(self, episode_id, elapsed):
        episode_id = np.asarray(episode_id, dtype=np.int64).reshape(self.N)
        elapsed = np.asarray(elapsed, dtype=np.int32).reshape(self.N)
        return ~self.stepped | (elapsed == 0) | (episode_id != self.last_id), episode_id

    def need(self, episode_id, elapsed):
        fresh, _ = self._fresh(episode_id, elapsed)
        if self.mode == 0:
            return np.ones(self.N, dtype=bool)
        return fresh | (self.count == 0)

    def _y(self, chunks):
        x = np.asarray(chunks, dtype=np.float32)
        if x.shape != (self.N, self.C, self.A):
            raise ValueError(f"chunks of shape {x.shape}, expected {(self.N, self.C, self.A)}")
        return x if self.mean is None else x * self.std + self.mean          # float32: a multiplication, then an addition

    def step(self, chunks, episode_id, elapsed):
        fresh, episode_id = self._fresh(episode_id, elapsed)
        N, C = self.N, self.C
        env = np.arange(N)
        if self.mode == 0:
            if chunks is None:
                raise ValueError("chunks: ensemble mode needs a chunk in every call")
            y = self._y(chunks)
            self.head[fresh] = 0
            self.count[fresh] = 0
            k = np.arange(C)[None, :]
            c = np.minimum(self.count[:, None], C - 1 - k)                       # [N, C]
            j = ((self.head[:, None] + k) % C)[:, :, None]
            old = np.take_along_axis(self.buf, j, axis=1)
            upd = (old * self.cum[np.maximum(c - 1, 0)][:, :, None] + y * self.w[c][:, :, None]) / self.cum[c][:, :, None]
            np.put_along_axis(self.buf, j, np.where((c == 0)[:, :, None], y, upd).astype(np.float32), axis=1)
            action = self.buf[env, self.head].copy()
            self.head = (self.head + 1) % C
            self.count = np.minimum(self.count + 1, C - 1)
        else:
            self.count[fresh] = 0
            need = self.count == 0
            action = np.zeros((N, self.A), dtype=np.float32)
            if chunks is not None:
                y = self._y(chunks)
                self.buf[need] = y[need, self.first:self.first + self.k]
                self.head[need] = 0
                self.count[need] = self.k
                starved = np.zeros(N, dtype=bool)
            else:
                starved = need
                self.starved += int(need.sum())
                self.prev[need & fresh] = 0
            run = ~starved
            action[run] = self.buf[env[run], self.head[run]]
            action[starved] = self.prev[starved]
            self.head[run] += 1
            self.count[run] -= 1
        self.prev = action.copy()
        self.stepped[:] = True
        self.last_id = episode_id.copy()
        assert action.dtype == np.float32
        return action


class ActionChunks:
    """Per-env chunk execution on the device (avsim_chunk_*): one state per handle, so one ActionChunks per env object at a time.
    env: anything that holds a device-I/O handle the way vec_env.VecEnv does (h, L, device, torch, num_envs, _bind_stream).  ensemble: None
    -> queue mode with n_action_steps (default: chunk_size) rows from row `first`; a coefficient -> LeRobot's temporal ensembling with
    ensemble_tables(chunk_size, coeff).  action_dim defaults to the env's joint count.  stats: CompressedDataset.stats()'s, whose "action"
    mean / std un-normalise the chunks; None: the chunks are actions already.  Every call runs on torch's current stream; need() and step()
    do not synchronise, starved() does.  ValueError for what the library refuses."""

    def __init__(self, env, chunk_size, action_dim=None, ensemble=None, n_action_steps=None, first=0, stats=None):
        from .images import check_call
        self._check = check_call
        self.env, self.torch = env, env.torch
        self.N, self.C = int(env.num_envs), int(chunk_size)
        self.A = int(action_dim if action_dim is not None else env.nj)
        mean = std = None
        if stats is not None:
            mean, std = stats["action"]["mean"], stats["action"]["std"]
        if ensemble is None:
            self.mode, tables = "queue", None
            n_action_steps = self.C if n_action_steps is None else n_action_steps
        else:
            self.mode = "ensemble"
            tables = ensemble_tables(self.C, ensemble) if 1 <= self.C <= MAX_CHUNK else None
        ms = mean_std(mean, std, self.A)
        self.setup_args = dict(mode=self.mode, tables=tables, n_action_steps=n_action_steps, first=first,
                               mean=None if ms is None else ms[0], std=None if ms is None else ms[1])
        env._bind_stream()
        self._check(env.h, env.L.avsim_chunk_setup(env.h.h, self.C, self.A, MODES[self.mode], int(n_action_steps or 0), int(first),
                                                   None if tables is None else tables.ctypes.data, None if ms is None else ms.ctypes.data))
        torch, dev = self.torch, env.device
        self._action = torch.zeros((self.N, self.A), dtype=torch.float32, device=dev)
        self._need = torch.zeros(self.N, dtype=torch.uint8, device=dev)
        self._any = torch.zeros(1, dtype=torch.int32, device=dev)

    def reference(self):
        """A ChunkReference with this object's set-up."""
        return ChunkReference(self.N, self.C, self.A, **self.setup_args)

    def _ids(self, info):
        torch, dev = self.torch, self.env.device
        eid, el = info["episode_id"], info["elapsed_steps"]
        assert isinstance(eid, torch.Tensor) and eid.dtype == torch.int64 and eid.device == dev and tuple(eid.shape) == (self.N,) and eid.is_contiguous(), \
            "info['episode_id']: a contiguous int64 [N] tensor on the env's device"
        assert isinstance(el, torch.Tensor) and el.dtype == torch.int32 and el.device == dev and tuple(el.shape) == (self.N,) and el.is_contiguous(), \
            "info['elapsed_steps']: a contiguous int32 [N] tensor on the env's device"
        return eid, el

    def need(self, info):
        """(need bool [N], any int32 [1]) on the device, overwritten by the next call: which envs need a chunk in the next step() given
        this info, and whether any does.  Changes no state; does not synchronise."""
        env = self.env
        env._bind_stream()
        eid, el = self._ids(info)
        self._check(env.h, env.L.avsim_chunk_need(env.h.h, eid.data_ptr(), el.data_ptr(), self._need.data_ptr(), self._any.data_ptr()))
        return self._need.view(self.torch.bool), self._any

    def step(self, chunks, info):
        """chunks: float32 [N, C, A] on the env's device (normalised when stats were given), or None in queue mode -> the action float32
        [N, A] for env.step, a preallocated tensor that the next call overwrites.  The chunk tensor is read before later work on the stream:
        the caller may overwrite it as soon as the call returns.  Does not synchronise."""
        env, torch = self.env, self.torch
        env._bind_stream()
        eid, el = self._ids(info)
        if chunks is not None:
            assert isinstance(chunks, torch.Tensor) and chunks.dtype == torch.float32 and chunks.device == env.device, "chunks: a float32 tensor on the env's device"
            assert tuple(chunks.shape) == (self.N, self.C, self.A), f"chunks of shape {tuple(chunks.shape)}, expected {(self.N, self.C, self.A)}"
            chunks = chunks.contiguous()
        self._check(env.h, env.L.avsim_chunk_step(env.h.h, None if chunks is None else chunks.data_ptr(), eid.data_ptr(), el.data_ptr(), self._action.data_ptr()))
        return self._action

    def reset(self):
        """All envs unstepped: every env is fresh in the next call.  Does not synchronise."""
        self.env._bind_stream()
        self._check(self.env.h, self.env.L.avsim_chunk_reset(self.env.h.h))

    def starved(self):
        """Env-calls that needed a chunk and got none since the set-up; synchronises."""
        c = np.zeros(1, dtype=np.uint64)
        self.env._bind_stream()
        self._check(self.env.h, self.env.L.avsim_chunk_starved(self.env.h.h, c.ctypes.data))
        return int(c[0])
