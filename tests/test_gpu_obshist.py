"""Per-env observation histories on the device (avsim_obs_history_*, csrc/avsim_obshist.hip; obshist.ObsHistory, BatchedSim.obs_history_*)
against their specification, av_aloha_amd.obshist.ObsHistoryReference.  Every history of every call is compared by np.array_equal on float32
arrays with no NaN on either side.  The handles are vector envs without cameras; no physics step is taken: observations, episode ids and
elapsed steps are tensors the tests write.  Inputs: random bytes, standard-normal states, fixed seeds."""
import ctypes
import time

import numpy as np
import pytest

from av_aloha_amd import images, imgprep
from av_aloha_amd import obshist as oh
from av_aloha_amd.sim import BatchedSim
from av_aloha_amd.vec_env import make_vec
from avsim_test_util import same
from gpu_util import torch as T

pytestmark = pytest.mark.gpu

PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
CAMS = ["a", "b"]
LUTS = {"a": imgprep.normalise_lut([0.4, 0.5, 0.6], [0.2, 0.25, 0.3]).astype(np.float32), "b": imgprep.identity_lut()}
# (source, crop, box of camera a, box of camera b, D, state statistics): 3 h w = 3, 30 (scalar), 36 (wide, a group of four straddles the rows of
# six), 1005 (odd: scalar), 12288 (wide) with the box on every border and strictly inside (x0 in 0..5, y0 in 0..3)
CONFIGS = [((1, 1), (1, 1), (0, 0, 0), (0, 0, 1), 0, False),
           ((2, 5), (2, 5), (0, 0, 0), (0, 0, 1), 1, True),
           ((3, 6), (2, 6), (0, 0, 1), (0, 1, 0), 21, False),
           ((5, 67), (5, 67), (0, 0, 0), (0, 0, 1), 21, True),
           ((35, 133), (32, 128), (0, 0, 0), (5, 3, 1), 1, False),
           ((35, 133), (32, 128), (5, 0, 1), (0, 3, 0), 0, False),
           ((35, 133), (32, 128), (2, 1, 0), (2, 1, 1), 21, True)]


@pytest.fixture(scope="module")
def envs():
    """vector envs by size, made once and shared: the history state is re-initialised by every set-up"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = make_vec(PEG, N, 50, cameras=[])
        return made[N]
    yield get
    for e in made.values():
        e.close()


def stats_for(D, seed=11):
    rng = np.random.default_rng(seed)
    return {"observation.state": {"mean": rng.standard_normal(D).astype(np.float32), "std": (rng.random(D) + 0.25).astype(np.float32)}}


def observations(calls, N, D, ncam, fmt, hw, seed):
    """(states float32 [calls, N, D], per camera the batches [calls, N, ...]): u8, or floats that are u / 255 for one half and anything in
    [-0.1, 1.1] for the other (the rounding and the clamp of imgprep.to_u8)"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((calls, N, D)).astype(np.float32)
    H, W = hw
    imgs = []
    for _ in range(ncam):
        u = rng.integers(0, 256, (calls, N, H, W, 3), dtype=np.uint8)
        if fmt == 0:
            imgs.append(u)
        else:
            f = np.ascontiguousarray((u.astype(np.float32) / np.float32(255)).transpose(0, 1, 4, 2, 3))
            other = (rng.random(f.shape) * 1.2 - 0.1).astype(np.float32)
            imgs.append(np.where(rng.random(f.shape) < 0.5, f, other).astype(np.float32))
    return s, imgs


def info_of(env, ids, elapsed):
    return {"episode_id": T.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(env.device),
            "elapsed_steps": T.from_numpy(np.ascontiguousarray(elapsed, dtype=np.int32)).to(env.device)}


def obs_of(env, hist, s, imgs, t):
    obs = {f"observation.images.{c}": T.from_numpy(imgs[i][t]).to(env.device) for i, c in enumerate(hist.cameras)}
    if hist.D > 0:
        obs["observation.state"] = T.from_numpy(s[t]).to(env.device)
    return obs


def check(hist, out, ref_out, where):
    sh, ih = ref_out
    assert set(out) == ({"observation.state"} if hist.D > 0 else set()) | {f"observation.images.{c}" for c in hist.cameras}
    if hist.D > 0:
        assert same(out["observation.state"].cpu().numpy(), sh), where
    for i, c in enumerate(hist.cameras):
        got = out[f"observation.images.{c}"].cpu().numpy()
        assert same(got, ih[i]), (where, c, np.argwhere(got != ih[i])[:4])


def run(env, hist, ref, s, imgs, ids, elapsed, t0=0):
    """calls t = t0 .. len(ids)-1; every history equal"""
    for t in range(t0, len(ids)):
        out = hist.push(obs_of(env, hist, s, imgs, t), info_of(env, ids[t], elapsed[t]))
        check(hist, out, ref.push(s[t] if hist.D > 0 else None, [im[t] for im in imgs], ids[t], elapsed[t]), t)


def fresh_schedule(N, calls):
    """env e is made fresh on call (e mod 5) + 1, in the way (e // 5) mod 5 names: by id change only, by elapsed == 0 only, by both, twice
    on consecutive calls, never.  (Call 0 starts every env: none has been pushed.)"""
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


def nan_fill(hist):
    for t in hist.out.values():
        t.fill_(float("nan"))


# ---- the passes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["gym", "lerobot"])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_histories_equal_the_specification(envs, K, fmt):
    """K + 4 calls: every slot has been shifted out once; env 2 starts anew on call 2 (id change), env 1 on call K + 1 (elapsed 0).  The
    histories hold NaN before the first call: a fresh env's lanes must not read them."""
    N, calls = 3, K + 4
    env = envs(N)
    ids = np.tile(np.arange(N, dtype=np.int64), (calls, 1))
    ids[2:, 2] += N
    elapsed = np.tile(np.arange(1, calls + 1, dtype=np.int32)[:, None], (1, N))
    elapsed[K + 1:, 1] -= K + 2
    for n, (src, crop, box_a, box_b, D, with_stats) in enumerate(CONFIGS):
        hist = oh.ObsHistory(env, K, stats=stats_for(D) if with_stats else None, crop=crop, cameras=CAMS, state_dim=D, fmt=fmt, size=src,
                             boxes={"a": box_a, "b": box_b}, luts=LUTS)
        nan_fill(hist)
        s, imgs = observations(calls, N, D, 2, oh.FORMATS[fmt], src, seed=100 * K + n)
        run(env, hist, hist.reference(), s, imgs, ids, elapsed)


@pytest.mark.parametrize("N", [70, 1100])
def test_large_batch_fresh_per_env(envs, N):
    """past one wave, and past the 1024 lanes of the bookkeeping kernel; fresh by id, by elapsed, by both, twice in a row, never"""
    K, D, calls = 3, 21, 9
    env = envs(N)
    ids, elapsed = fresh_schedule(N, calls)
    for fmt in ("gym", "lerobot") if N == 70 else ("gym",):
        hist = oh.ObsHistory(env, K, stats=stats_for(D), cameras=["a"], state_dim=D, fmt=fmt, size=(2, 5), luts=LUTS)
        nan_fill(hist)
        s, imgs = observations(calls, N, D, 1, oh.FORMATS[fmt], (2, 5), seed=N)
        run(env, hist, hist.reference(), s, imgs, ids, elapsed)


@pytest.mark.parametrize("fmt", ["gym", "lerobot"])
def test_one_step_is_prep_images(envs, fmt):
    N, src, crop = 3, (35, 133), (32, 128)
    env = envs(N)
    st = {"observation.images.a": {"mean": np.array([0.4, 0.5, 0.6], np.float32), "std": np.array([0.2, 0.25, 0.3], np.float32)}}
    hist = oh.ObsHistory(env, 1, stats=st, crop=crop, cameras=["a"], state_dim=0, fmt=fmt, size=src)
    _, imgs = observations(2, N, 0, 1, oh.FORMATS[fmt], src, seed=3)
    lut = T.from_numpy(LUTS["a"].reshape(1, 3, 256)).to(env.device)
    x0, y0 = imgprep.center_box(src, crop)
    for t in range(2):
        img = T.from_numpy(imgs[0][t]).to(env.device)
        got = hist.push({"observation.images.a": img}, info_of(env, [0, 1, 2], [t + 1] * 3))["observation.images.a"].cpu().numpy()
        want = env.prep_images(img, lut, [(x0, y0, 0)] * N, crop).cpu().numpy()
        assert got.shape == (N, 1, 3) + crop and same(got[:, 0], want), t


def test_an_unaligned_history_takes_the_scalar_path(envs):
    """3 h w is a multiple of four but the history starts 4 bytes off a 16-byte boundary: single floats, the same values"""
    N, K, src, crop = 3, 3, (35, 133), (32, 128)
    env = envs(N)
    hist = oh.ObsHistory(env, K, crop=crop, cameras=["a"], state_dim=0, fmt="gym", size=src, boxes={"a": (5, 3, 1)}, luts=LUTS)
    ref = hist.reference()
    n = N * K * 3 * crop[0] * crop[1]
    flat = T.full((n + 4,), float("nan"), dtype=T.float32, device=env.device)
    off = 1 + (-(flat.data_ptr() // 4) % 4)                      # the first float one past a 16-byte boundary
    view = flat[off:off + n].view(N, K, 3, *crop)
    assert view.data_ptr() % 16 == 4
    _, imgs = observations(K + 2, N, 0, 1, 0, src, seed=8)
    for t in range(K + 2):
        img = T.from_numpy(imgs[0][t]).to(env.device)
        info = info_of(env, [0, 1, 2], [t + 1] * 3)
        src_p, dst_p = (ctypes.c_void_p * 1)(img.data_ptr()), (ctypes.c_void_p * 1)(view.data_ptr())
        env._bind_stream()
        images.check_call(env.h, env.L.avsim_obs_history_push(env.h.h, info["episode_id"].data_ptr(), info["elapsed_steps"].data_ptr(), None, None, src_p, dst_p))
        _, ih = ref.push(None, [imgs[0][t]], [0, 1, 2], [t + 1] * 3)
        assert same(view.cpu().numpy(), ih[0]), t
    edge = flat.cpu().numpy()
    assert np.isnan(edge[:off]).all() and np.isnan(edge[off + n:]).all()          # nothing written outside the history


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def raw_setup(env, K, D, ms, ncam, fmt, H, W, lut, box, h, w):
    env._bind_stream()
    images.check_call(env.h, env.L.avsim_obs_history_setup(env.h.h, K, D, None if ms is None else ms.ctypes.data, ncam, fmt, H, W,
                                                           None if lut is None else lut.ctypes.data, None if box is None else box.ctypes.data, h, w))


def test_refusals_leave_the_state_alone(envs):
    N, K, D, src, crop = 3, 2, 3, (3, 6), (2, 6)
    env = envs(N)
    lut = np.ascontiguousarray(np.stack([LUTS["a"], LUTS["b"]]), dtype=np.float32)
    box = np.array([[0, 0, 1], [0, 1, 0]], dtype=np.int32)
    ms = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.float32)

    def bad_ms(i, j, v):
        b = ms.copy()
        b[i, j] = v
        return b

    def bad_box(c, j, v):
        b = box.copy()
        b[c, j] = v
        return b
    ok = (K, D, ms, 2, 0, 3, 6, lut, box, 2, 6)

    def but(**kw):
        names = ["K", "D", "ms", "ncam", "fmt", "H", "W", "lut", "box", "h", "w"]
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    refused = [but(K=0), but(K=17), but(D=-1), but(D=257, ms=None), but(ncam=-1), but(ncam=9), but(D=0, ms=None, ncam=0), but(fmt=2), but(fmt=-1),
               but(H=0), but(W=65536), but(h=0), but(w=65536), but(h=4), but(w=7), but(box=bad_box(0, 0, 1)), but(box=bad_box(1, 1, 2)),
               but(box=bad_box(0, 1, -1)), but(box=bad_box(1, 2, 2)), but(box=bad_box(0, 2, -1)), but(lut=None), but(box=None),
               but(ms=bad_ms(0, 1, np.nan)), but(ms=bad_ms(0, 0, np.inf)), but(ms=bad_ms(1, 2, 0.0)), but(ms=bad_ms(1, 0, np.nan)), but(ms=bad_ms(1, 1, -np.inf))]
    calls = 2 + len(refused) + 4
    ids = np.tile(np.arange(N, dtype=np.int64), (calls, 1))
    elapsed = np.tile(np.arange(1, calls + 1, dtype=np.int32)[:, None], (1, N))
    hist = oh.ObsHistory(env, K, stats={"observation.state": {"mean": ms[0], "std": ms[1]}}, crop=crop, cameras=CAMS, state_dim=D, fmt="gym", size=src,
                         boxes={"a": box[0], "b": box[1]}, luts=LUTS)
    ref = hist.reference()
    s, imgs = observations(calls, N, D, 2, 0, src, seed=2)
    run(env, hist, ref, s, imgs, ids[:2], elapsed[:2])
    for i, r in enumerate(refused):
        with pytest.raises(ValueError):
            raw_setup(env, *r)
        run(env, hist, ref, s, imgs, ids[:3 + i], elapsed[:3 + i], t0=2 + i)          # as if the refused call had not happened
    # the refusals of push: a NULL state, a NULL history, a NULL camera pointer, no pointer tables, no ids
    t = 2 + len(refused)
    obs, info = obs_of(env, hist, s, imgs, t), info_of(env, ids[t], elapsed[t])
    eid, el, st = info["episode_id"].data_ptr(), info["elapsed_steps"].data_ptr(), obs["observation.state"].data_ptr()
    sh = hist.out["observation.state"].data_ptr()
    src_p = (ctypes.c_void_p * 2)(*[obs[f"observation.images.{c}"].data_ptr() for c in CAMS])
    dst_p = (ctypes.c_void_p * 2)(*[hist.out[f"observation.images.{c}"].data_ptr() for c in CAMS])
    hole_s, hole_d = (ctypes.c_void_p * 2)(src_p[0], None), (ctypes.c_void_p * 2)(None, dst_p[1])
    push = env.L.avsim_obs_history_push
    for n, args in enumerate([(eid, el, None, sh, src_p, dst_p), (eid, el, st, None, src_p, dst_p), (eid, el, st, sh, hole_s, dst_p), (eid, el, st, sh, src_p, hole_d),
                              (eid, el, st, sh, None, dst_p), (eid, el, st, sh, src_p, None), (None, el, st, sh, src_p, dst_p), (eid, None, st, sh, src_p, dst_p)]):
        with pytest.raises(ValueError):
            images.check_call(env.h, push(env.h.h, *args))
        if n % 3 == 2:
            run(env, hist, ref, s, imgs, ids[:t + 1], elapsed[:t + 1], t0=t)
            t += 1
    run(env, hist, ref, s, imgs, ids[:t + 1], elapsed[:t + 1], t0=t)
    T.cuda.synchronize()


def test_calls_before_the_setup_are_refused():
    env = make_vec(PEG, 2, 10, cameras=[])
    try:
        L, h = env.L, env.h.h
        info = info_of(env, [0, 1], [0, 0])
        s, sh = T.zeros((2, 3), dtype=T.float32, device=env.device), T.zeros((2, 2, 3), dtype=T.float32, device=env.device)
        for rc in (L.avsim_obs_history_reset(h),
                   L.avsim_obs_history_push(h, info["episode_id"].data_ptr(), info["elapsed_steps"].data_ptr(), s.data_ptr(), sh.data_ptr(), None, None)):
            with pytest.raises(ValueError):
                images.check_call(env.h, rc)
        hist = oh.ObsHistory(env, 2, state_dim=3)                    # ... and after it they are not
        out = hist.push({"observation.state": s + 1}, info)
        assert same(out["observation.state"].cpu().numpy(), np.ones((2, 2, 3), np.float32))
    finally:
        env.close()


def test_a_second_setup_and_reset_start_over(envs):
    N, D = 3, 2
    env = envs(N)
    calls = 7
    ids = np.tile(np.arange(N, dtype=np.int64), (calls, 1))
    elapsed = np.tile(np.arange(1, calls + 1, dtype=np.int32)[:, None], (1, N))
    s, imgs = observations(calls, N, D, 1, 0, (2, 5), seed=9)
    hist = oh.ObsHistory(env, 4, cameras=["a"], state_dim=D, fmt="gym", size=(2, 5))
    run(env, hist, hist.reference(), s, imgs, ids[:2], elapsed[:2])
    hist = oh.ObsHistory(env, 3, cameras=["a"], state_dim=D, fmt="gym", size=(2, 5))          # the same ids and elapsed > 0: fresh all the same
    ref = hist.reference()
    nan_fill(hist)
    run(env, hist, ref, s, imgs, ids[:4], elapsed[:4], t0=2)
    hist.reset()
    ref.reset()
    out = hist.push(obs_of(env, hist, s, imgs, 4), info_of(env, ids[4], elapsed[4]))
    assert same(out["observation.state"].cpu().numpy(), np.repeat(s[4][:, None], 3, axis=1))
    check(hist, out, ref.push(s[4], [imgs[0][4]], ids[4], elapsed[4]), 4)
    run(env, hist, ref, s, imgs, ids, elapsed, t0=5)


# ---- the stream ----------------------------------------------------------------------------------------------------------------------
def test_back_to_back_pushes_with_the_sources_overwritten(envs):
    """twenty calls with no host wait in between; the source tensors are overwritten as soon as each call has returned"""
    N, K, D, calls, src = 70, 3, 21, 20, (3, 6)
    env = envs(N)
    ids, elapsed = fresh_schedule(N, calls)
    s, imgs = observations(calls + 1, N, D, 1, 0, src, seed=4)
    sd, imd = T.from_numpy(s).to(env.device), T.from_numpy(imgs[0]).to(env.device)
    infos = [info_of(env, ids[t], elapsed[t]) for t in range(calls)]
    hist = oh.ObsHistory(env, K, stats=stats_for(D), crop=(2, 6), cameras=["a"], state_dim=D, fmt="gym", size=src, luts=LUTS)
    ref = hist.reference()
    bs, bi, got = sd[0].clone(), imd[0].clone(), []
    T.cuda.synchronize()
    for t in range(calls):
        out = hist.push({"observation.state": bs, "observation.images.a": bi}, infos[t])
        got.append({k: v.clone() for k, v in out.items()})
        bs.copy_(sd[t + 1])
        bi.copy_(imd[t + 1])
    T.cuda.synchronize()
    for t in range(calls):
        check(hist, got[t], ref.push(s[t], [imgs[0][t]], ids[t], elapsed[t]), t)


def test_push_and_reset_do_not_synchronise(envs):
    N, K, D, src = 70, 3, 21, (3, 6)
    env = envs(N)
    hist = oh.ObsHistory(env, K, cameras=["a"], state_dim=D, fmt="gym", size=src)
    s, imgs = observations(1, N, D, 1, 0, src, seed=5)
    obs, info = obs_of(env, hist, s, imgs, 0), info_of(env, np.arange(N), np.ones(N))
    hist.push(obs, info)
    T.cuda.synchronize()
    st = T.cuda.current_stream()
    t0 = time.perf_counter()
    T.cuda._sleep(int(2e9))            # about a second of GPU time in front of the calls
    hist.push(obs, info)
    hist.reset()
    hist.push(obs, info)
    busy = not st.query()
    dt = time.perf_counter() - t0
    T.cuda.synchronize()
    assert busy and dt < 0.3, (busy, dt)


# ---- host I/O ------------------------------------------------------------------------------------------------------------------------
def test_batched_sim_host_io():
    N, K, D, calls, src, crop = 5, 3, 21, 8, (3, 6), (2, 6)
    sim = BatchedSim("insert_peg", 3, N)
    try:
        ids, elapsed = fresh_schedule(N, calls)
        lut = np.stack([LUTS["a"], LUTS["b"]])
        st = stats_for(D)["observation.state"]
        for fmt in (0, 1):
            s, imgs = observations(calls, N, D, 2, fmt, src, seed=6 + fmt)
            kw = sim.obs_history_setup(K, D, mean=st["mean"], std=st["std"], fmt=fmt, src_hw=src, out_hw=crop, lut=lut, box=[(0, 0, 1), (0, 1, 0)])
            ref = oh.ObsHistoryReference(N, K, D, **kw)
            for t in range(calls):
                sh, ih = sim.obs_history_push(s[t], [im[t] for im in imgs], ids[t], elapsed[t])
                rs, ri = ref.push(s[t], [im[t] for im in imgs], ids[t], elapsed[t])
                assert same(sh, rs) and same(ih[0], ri[0]) and same(ih[1], ri[1]), (fmt, t)
                if t == 4:
                    sim.obs_history_reset()
                    ref.reset()
        ref = oh.ObsHistoryReference(N, 2, 4, **sim.obs_history_setup(2, 4))          # a state alone
        x = np.arange(N * 4, dtype=np.float32).reshape(N, 4)
        for t in range(3):
            assert same(sim.obs_history_push(x + t, None, ids[0], elapsed[0] + t)[0], ref.push(x + t, None, ids[0], elapsed[0] + t)[0])
        with pytest.raises(ValueError):
            sim.obs_history_setup(0)
        with pytest.raises(ValueError):
            sim.obs_history_push(x[:, :3], None, ids[0], elapsed[0])
    finally:
        sim.close()
