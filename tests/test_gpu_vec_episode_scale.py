"""The episode bookkeeping of the vector env (avsim_episode_*, k_episode) at batch scale: past one wave (N = 65), past one chunk of 1024
envs (N = 1025) and with the chunk carry taken twice (N = 2051), in host-pointer mode and through VecEnv, against the host model
(tests/vec_episode_model.py) and a plain BatchedSim twin stepped in lock step.  Everything is compared exactly: ids and flags as
integers, agent_pos / reward / success bit for bit (an env's physics does not depend on its neighbours:
test_gpu_bench_path.test_ragged_batch_sizes_give_the_same_envs).

The twin and the model run first, once per (N, precision, terminate_on_success), and leave the list of calls with the outputs expected
of each; the handle under test then replays that list.  The model's `diverged` input is the twin's diag bit, never the handle's."""
import numpy as np
import pytest

from av_aloha_amd import _ffi
from av_aloha_amd.constants import SIM_PHYSICS_ENV_STEP_RATIO
from av_aloha_amd.sim import BatchedSim, load_blob
from av_aloha_amd.vec_env import OBJECT_BOXES, VecEnv, make_vec, sample_poses
from avsim_test_util import host_observe
from gpu_util import torch as T
from vec_episode_model import INSERT_BEFORE, MAX_STEPS, POKE_BEFORE, EpisodeModel, check_invariants, coverage, scenario

pytestmark = pytest.mark.gpu

TASK, SEED = "slot_insertion", 11
PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
SLOT_IN, STICK_IN = [0.0, 0.12, 0.0], [0.0, 0.12, 0.0005]        # test_gpu_physics.test_staged_rewards_and_success_match_the_oracle's "inserted"
KEPT = ("elapsed", "reward", "success", "terminated", "truncated")      # what VecEnv.reset leaves of the last step for the envs it does not restart


# ---- the reference: twin + model -----------------------------------------------------------------------------------------------------

_REFS = {}


def reference(N, f64, tos):
    """{"ops": the calls of the scenario with the outputs expected of each, "cap": log capacity = started // 2, "log": the model's
    records below it, "started", "cov": the coverage figures}; computed once and not changed afterwards."""
    key = (N, f64, tos)
    if key in _REFS:
        return _REFS[key]
    sc = scenario(N, 100 + N)
    twin = BatchedSim(TASK, 3, N, f64=f64, options={"solver": 1})
    big = N * (sc["calls"] + 4)                      # more than can start: every record is kept, the cap is applied below
    m = EpisodeModel(TASK, N, SEED, MAX_STEPS, tos, big)
    last = {k: np.zeros(N, dtype=np.int64) for k in KEPT}
    ops = []

    def reset(mask):
        out = m.reset(mask)
        twin.reset(m.poses(), mask=out["start"])
        for k in KEPT:
            last[k] = np.where(out["start"], 0, last[k])
        ops.append(("reset", mask, {"agent_pos": host_observe(twin), "id": out["id"], "count": m.count(), **last}))

    reset(None)
    base = ops[0][2]["agent_pos"].astype(np.float32)
    rng = np.random.default_rng(sc["action_seed"])
    for call in range(1, sc["calls"] + 1):
        if call == INSERT_BEFORE:
            q, _, _, _ = twin.get_state()
            q[sc["inserted"], 23:26], q[sc["inserted"], 30:33] = SLOT_IN, STICK_IN
            twin.set_qpos(q)
            ops.append(("insert", sc["inserted"], None))
        if call in sc["masks"]:
            reset(sc["masks"][call])
        if call == POKE_BEFORE:
            _, v, _, _ = twin.get_state()
            v[sc["poke"], 30] = 1e9
            twin.set_state(qvel=v)
            ops.append(("poke", sc["poke"], None))
        if call == 10:
            ops.append(("refused", None, None))
        a = (base + rng.normal(0, 0.05, base.shape)).astype(np.float32)
        ap, rw, su = twin.step(a)
        div = (twin.diag()[:, 3] & 1) != 0             # (read before the twin's reset / observe launches write diag again)
        out = m.step(rw, su, div)
        if out["start"].any():
            twin.reset(m.poses(), mask=out["start"])
            ap = np.where(out["start"][:, None], host_observe(twin), ap)
        for k in KEPT:
            last[k] = out[k].astype(np.int64)
        ops.append(("step", a, {"agent_pos": ap, "id": out["id"], "count": m.count(), **last}))
    twin.close()
    check_invariants(m)
    cap = m.started // 2
    m.log_cap = cap
    log = {k: x[:cap] for k, x in m.log(cap).items()}
    _REFS[key] = {"ops": ops, "cap": cap, "log": log, "started": m.started, "cov": coverage(m, N), "sc": sc}
    return _REFS[key]


# ---- the two ways to the handle under test -------------------------------------------------------------------------------------------

class HostPointers:
    """A handle without AVSIM_IO_DEVICE, driven through ctypes with numpy arrays (outputs staged through the handle's scratch slots)."""

    def __init__(self, N, f64, tos):
        blob, _ = load_blob(TASK, 3)
        self.N, self.tos = N, tos
        self.h = h = _ffi.Handle(blob, N, 0, _ffi.AVSIM_F64_PHYSICS if f64 else 0)
        self.L = h.L
        h.check(self.L.avsim_set_option(h.h, b"solver", 1.0))
        self.box = np.ascontiguousarray(OBJECT_BOXES[TASK][0], dtype=np.float64)
        self.share = np.ascontiguousarray(OBJECT_BOXES[TASK][1], dtype=np.int32)

    def setup(self, cap):
        self.h.check(self.L.avsim_episode_setup(self.h.h, self.box.ctypes.data, self.share.ctypes.data, SEED, MAX_STEPS, int(self.tos), cap))

    def reset(self, mask, skip=()):
        N = self.N
        out = {"agent_pos": np.full((N, self.h.nj), np.nan), "id": np.full(N, -7, dtype=np.int64)}
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        p = {k: (None if k in skip else v.ctypes.data) for k, v in out.items()}
        self.h.check(self.L.avsim_episode_reset(self.h.h, _ffi.ptr(m), p["agent_pos"], p["id"]))
        return {k: v for k, v in out.items() if k not in skip}

    def step(self, a, skip=()):
        N = self.N
        out = {"agent_pos": np.full((N, self.h.nj), np.nan), "reward": np.full(N, -7, dtype=np.int32), "success": np.full(N, 7, dtype=np.uint8),
               "terminated": np.full(N, 7, dtype=np.uint8), "truncated": np.full(N, 7, dtype=np.uint8), "id": np.full(N, -7, dtype=np.int64),
               "elapsed": np.full(N, -7, dtype=np.int32)}
        p = {k: (None if k in skip else v.ctypes.data) for k, v in out.items()}
        self.h.check(self.L.avsim_episode_step(self.h.h, a.ctypes.data, SIM_PHYSICS_ENV_STEP_RATIO, p["agent_pos"], p["reward"], p["success"],
                                               p["terminated"], p["truncated"], p["id"], p["elapsed"]))
        return {k: v for k, v in out.items() if k not in skip}

    def insert(self, envs):
        q = np.empty((self.N, self.h.nq))
        self.h.check(self.L.avsim_get_state(self.h.h, q.ctypes.data, None, None, None))
        q[envs, 23:26], q[envs, 30:33] = SLOT_IN, STICK_IN
        self.h.check(self.L.avsim_set_qpos(self.h.h, q.ctypes.data))

    def poke(self, envs):
        v = np.empty((self.N, self.h.nv))
        self.h.check(self.L.avsim_get_state(self.h.h, None, v.ctypes.data, None, None))
        v[envs, 30] = 1e9
        self.h.check(self.L.avsim_set_state(self.h.h, None, v.ctypes.data, None, None))

    def count(self):
        c = np.full(2, -7, dtype=np.int64)
        self.h.check(self.L.avsim_episode_count(self.h.h, c.ctypes.data))
        return int(c[0]), int(c[1])

    def log(self, n):
        ret, length = np.full(n, np.nan), np.full(n, -7, dtype=np.int32)
        mr, su = np.full(n, -7, dtype=np.int32), np.full(n, 7, dtype=np.uint8)
        obj = np.full((n, self.h.nobj, 7), np.nan)
        self.h.check(self.L.avsim_episode_log(self.h.h, n, ret.ctypes.data, length.ctypes.data, mr.ctypes.data, su.ctypes.data, obj.ctypes.data))
        return {"return": ret, "length": length, "max_reward": mr, "success": su, "obj_qpos0": obj}

    def sample(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        out = np.full((len(ids), self.h.nobj, 7), np.nan)
        self.h.check(self.L.avsim_sample_poses(self.h.h, SEED, len(ids), ids.ctypes.data, out.ctypes.data))
        return out

    def close(self):
        self.h.close()


class ThroughVecEnv:
    """Device mode: VecEnv's reset (reset_mask, the masked_fill_ of the kept outputs), step, start_log, episode_count, episode_log."""

    def __init__(self, N, f64, tos):
        self.N = N
        self.env = VecEnv(TASK, 3, N, MAX_STEPS, cameras=(), obs_format="gym", seed=SEED, terminate_on_success=tos, f64=f64, options={"solver": 1})

    def setup(self, cap):
        self.env.start_log(cap)

    def _kept(self, info, r, te, tr):
        return {"elapsed": info["elapsed_steps"], "reward": r, "success": info["is_success"], "terminated": te, "truncated": tr}

    def reset(self, mask, skip=()):
        env = self.env
        obs, info = env.reset(options=None if mask is None else {"reset_mask": T.as_tensor(mask)})
        out = {"agent_pos": obs["agent_pos"], "id": info["episode_id"], **self._kept(info, env._reward, env._term, env._trunc)}
        return {k: v.cpu().numpy().copy() for k, v in out.items()}

    def step(self, a, skip=()):
        env = self.env
        obs, r, te, tr, info = env.step(T.as_tensor(a, device=env.device))
        out = {"agent_pos": obs["agent_pos"], "id": info["episode_id"], **self._kept(info, r, te, tr)}
        return {k: v.cpu().numpy().copy() for k, v in out.items()}

    def _state(self, which):
        h = self.env.h
        x = T.empty((self.N, h.nq if which == 0 else h.nv), dtype=T.float64, device=self.env.device)
        args = [None] * 4
        args[which] = x.data_ptr()
        h.check(h.L.avsim_get_state(h.h, *args))
        return x, args

    def insert(self, envs):
        h = self.env.h
        q, args = self._state(0)
        i = T.as_tensor(np.flatnonzero(envs), device=q.device)
        q[i, 23:26] = T.tensor(SLOT_IN, dtype=T.float64, device=q.device)
        q[i, 30:33] = T.tensor(STICK_IN, dtype=T.float64, device=q.device)
        h.check(h.L.avsim_set_qpos(h.h, q.data_ptr()))

    def poke(self, envs):
        h = self.env.h
        v, args = self._state(1)
        v[T.as_tensor(envs, device=v.device), 30] = 1e9
        h.check(h.L.avsim_set_state(h.h, *args))

    def count(self):
        return self.env.episode_count()

    def log(self, n):
        g = self.env.episode_log(n)
        return {"return": g["return"], "length": g["length"], "max_reward": g["max_reward"], "success": g["success"].astype(np.uint8),
                "obj_qpos0": g["initial_object_poses"]}

    def sample(self, ids):
        return self.env.sample_poses(ids)

    def close(self):
        self.env.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------

def same(got, want, where):
    for k, g in got.items():
        w = np.asarray(want[k])
        g = np.asarray(g)
        g, w = (g, w) if g.dtype.kind == "f" else (g.astype(np.int64), w.astype(np.int64))      # (flags come as uint8 or bool)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{where}: {k} differs in {len(bad)} entries, first at {bad[:6].tolist()}: got {g[tuple(bad[0])]!r}, expected {w[tuple(bad[0])]!r}")


def check_coverage(ref, N, tos):
    cov = ref["cov"]
    print(f"N={N} tos={tos}: started {ref['started']}, log capacity {ref['cap']}, coverage {cov}")
    if N >= 65:
        assert cov["wave_split_calls"] >= 5, cov
    if N >= 1025:
        assert cov["chunk_split_calls"] >= 5, cov
    if tos:
        assert cov["terminated"] >= 20, cov
    else:
        assert cov["terminated"] == 0, cov
    assert cov["diverged"] >= min(2, N), cov
    assert cov["ended_below_cap"] > 0 and cov["ended_at_or_above_cap"] > 0, cov


def drive(adapter_cls, N, f64, tos):
    ref = reference(N, f64, tos)
    check_coverage(ref, N, tos)
    cap, nulls = ref["cap"], adapter_cls is HostPointers
    ad = adapter_cls(N, f64, tos)
    try:
        ad.setup(cap)
        assert ad.count() == (0, 0)
        call = 0
        for kind, arg, want in ref["ops"]:
            if kind == "insert":
                ad.insert(arg)
            elif kind == "poke":
                ad.poke(arg)
            elif kind == "refused":
                # more records than are kept: refused with a message; the calls that follow show that the handle still steps
                with pytest.raises(_ffi.AvsimError, match="records asked"):
                    ad.log(cap + 1)
            elif kind == "reset":
                # (host pointers: once without agent_pos -- the ids still come, and the next step's agent_pos is checked as ever)
                got = ad.reset(arg, skip=("agent_pos",) if nulls and call == 7 else ())
                same(got, want, f"reset before call {call + 1}")
                assert ad.count() == want["count"], (call, ad.count(), want["count"])
            else:
                call += 1
                # host pointers: calls 5 and 6 (truncations, the divergence) with NULL for reward and terminated, call 12 with NULL for all but one
                skip = () if not nulls else {5: ("reward", "terminated"), 6: ("reward", "terminated"),
                                             12: ("agent_pos", "reward", "success", "terminated", "truncated", "elapsed")}.get(call, ())
                same(ad.step(arg, skip=skip), want, f"step call {call}")
                assert ad.count() == want["count"], (call, ad.count(), want["count"])
        # the records, field for field (length 0 and zeros for the ids that have not finished)
        log, mlog = ad.log(cap), ref["log"]
        assert (mlog["length"] > 0).any() and (mlog["length"] == 0).any()
        same(log, mlog, "episode_log")
        done = mlog["length"] > 0
        assert np.array_equal(log["obj_qpos0"][done], sample_poses(TASK, SEED, np.flatnonzero(done)))
        with pytest.raises(_ffi.AvsimError, match="records asked"):
            ad.log(cap + 1)
        assert ad.count() == ref["ops"][-1][2]["count"] and ad.count()[0] == ref["started"]
        # the sampler on the handle for every id handed out
        ids = np.arange(ref["started"])
        assert np.array_equal(ad.sample(ids), sample_poses(TASK, SEED, ids))
        # a fresh set-up on the same handle: ids from 0, no records
        ad.setup(cap)
        assert ad.count() == (0, 0)
        log = ad.log(cap)
        assert not any(np.asarray(v).any() for v in log.values())
        first = ref["ops"][0][2]
        same(ad.reset(None), {**first, "count": None}, "reset after a fresh set-up")
        assert ad.count() == (N, 0)
    finally:
        ad.close()


@pytest.mark.parametrize("N,tos", [(1, False), (65, False), (1025, False), (1025, True), (2051, False), (2051, True)])
def test_host_pointer_episodes_match_the_model_and_the_twin(N, tos):
    """Host-pointer mode (never called by VecEnv).  Regimes of k_episode: 65 = the second wave (wsum), 1025 = the second chunk with one
    live lane, 2051 = three chunks (base_s carried twice, fin_s added up over them); 1 = the degenerate batch."""
    drive(HostPointers, N, False, tos)


def test_host_pointer_episodes_f64():
    drive(HostPointers, 65, True, False)


def test_vec_env_episodes_match_the_model_and_the_twin():
    """Device mode through VecEnv at the second chunk: reset(options={"reset_mask": ...}) with its masked_fill_ of the kept outputs,
    start_log, episode_count, episode_log."""
    drive(ThroughVecEnv, 1025, False, True)


def test_evaluate_vec_records_do_not_depend_on_the_batch_across_a_chunk():
    """test_gpu_vec_env's 3 / 4 / 10 check carried over the wave and the chunk boundary: 1100 episodes on 1030 envs (ids 1024 .. 1029 start
    in the second chunk, 1030 .. 1099 in the second round) and on 10 envs give the same record for every id."""
    from av_aloha_amd.harness import evaluate_vec

    def policy(obs, info):
        s = obs["observation.state"]
        ph = 0.5 * info["elapsed_steps"].to(T.float32) + info["episode_id"].to(T.float32)
        a = s.clone()
        a[:, :6] += 0.05 * T.sin(ph)[:, None]
        return a

    recs = []
    for N in (1030, 10):
        env = make_vec(PEG, N, 4, cameras=[], seed=9)
        recs.append(evaluate_vec(env, policy, 1100))
        env.close()
    for r in recs:
        assert [x["episode_id"] for x in r] == list(range(1100)) and all(x["length"] == 4 for x in r)
    want = sample_poses("insert_peg", 9, np.arange(1100))
    for k, (x, y) in enumerate(zip(*recs)):
        assert x["return"] == y["return"] and x["max_reward"] == y["max_reward"] and x["success"] == y["success"], k
        assert np.array_equal(x["initial_object_poses"], y["initial_object_poses"]) and np.array_equal(x["initial_object_poses"], want[k]), k
