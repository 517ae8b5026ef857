"""The paths on which a handle frees a device buffer and allocates a larger (or another) one, or sets a Host up a second time: every case drives one
handle through the sizes and compares each result, byte for byte, with the same call on a fresh handle -- which allocated once, at the size of that
call.  A buffer that grew too little, kept a stale capacity or lost a side effect of its reallocation (a stale shadow map, kernel arguments that
still point at freed memory) shows as a difference, or as a fault.

Shapes: the smallest at which each path is taken -- slot_insertion, 3 envs in different states, images of 48 x 64 (two tiles of 32 across, more than
one bin row).  The last test reads the two kernel timers across a fold of their event lists (csrc/avsim_dev.h EV_RING = 1024 pairs)."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TASK, N, H, W = "slot_insertion", 3, 48, 64
CAMS = ["zed_cam_left", "wrist_cam_right", "overhead_cam"]
OBJ = np.array([[0, 0.12, 0, 1, 0, 0, 0], [0, -0.05, 0, 1, 0, 0, 0.0]])
EV_RING = 1024


def make(n=N, **options):
    """A fresh handle whose envs differ: the objects shifted per env, and two control steps so that the arms have left the home pose."""
    from av_aloha_amd.sim import BatchedSim
    sim = BatchedSim(TASK, 3, n, options=options or None)
    obj = np.repeat(OBJ[None], n, 0)
    obj[:, :, 0] += 0.02 * np.arange(n)[:, None]
    sim.reset(obj)
    sim.step_ctrl()
    sim.step_ctrl()
    return sim


def moved(sim, k):
    """The state with the first arm's two shoulder joints turned by k steps: what a shadow map of the state before does not fit."""
    q = sim.get_state()[0].copy()
    q[:, 0] += 0.25 * k
    q[:, 1] -= 0.15 * k
    return q


def state_bytes(sim):
    return b"".join(a.tobytes() for a in sim.get_state()) + sim.get_latch().tobytes()


def test_depth_and_proxy_colour_scratch_grows_with_cameras_and_chunk():
    """One camera, three cameras, then chunks of one env with three cameras and of three envs with one: the last pair keeps chunk x cameras and
    triples the chunk -- the per-chunk counts (16 camera slots an env) must grow although the per-view buffers need not.  On the handle that
    has seen it all, and on one that starts at the small chunk."""
    def check(sim, chunk, cams):
        ref = make()
        if chunk:
            sim.set_option("render_chunk", chunk)
            ref.set_option("render_chunk", chunk)
        want_d, want_c = ref.render_depth(cams, H, W), ref.render_rgb(cams, H, W, visual=False)
        assert np.isfinite(want_d).all() and want_d.std() > 0 and want_c.std() > 0 and not np.array_equal(want_d[0], want_d[1])
        assert sim.render_depth(cams, H, W).tobytes() == want_d.tobytes(), (chunk, cams)
        assert sim.render_rgb(cams, H, W, visual=False).tobytes() == want_c.tobytes(), (chunk, cams)
        ref.close()
    sim = make()
    for chunk, cams in ((None, CAMS[:1]), (None, CAMS), (1, CAMS), (3, CAMS[:1])):
        check(sim, chunk, cams)
    sim.close()
    sim = make(render_chunk=1)
    for chunk, cams in ((1, CAMS), (3, CAMS[:1]), (3, CAMS)):
        check(sim, chunk, cams)
    sim.close()


def test_visual_scene_slots_flags_and_shadow_maps_regrow():
    """Three views, then nine: more scratch slots and flag rows.  Then shadows with maps of 512, 1024 and 512 texels, the arms moved before each:
    a map that was kept across its reallocation, or across the change of size, is the one of another state."""
    def check(sim, cams, q=None, **options):
        ref = make()
        for s in (sim, ref):
            for k, v in options.items():
                s.set_option(k, v)
            if q is not None:
                s.set_qpos(q)
        want = ref.render_rgb(cams, H, W)
        assert want.std() > 0 and ref.visual_info()["overflow"] == 0
        got = sim.render_rgb(cams, H, W)
        assert got.tobytes() == want.tobytes(), (cams, options)
        ref.close()
        return got
    sim = make()
    check(sim, CAMS[:1])
    plain = check(sim, CAMS)
    lit = [check(sim, CAMS[:2], q=moved(sim, k + 1), render_shadows=1, render_shadow_size=size) for k, size in enumerate((512, 1024, 512))]
    assert not np.array_equal(lit[0], lit[2]) and not np.array_equal(lit[0], plain[:, :2])          # (the arms did move, the shadows are there)
    sim.close()


def test_jpeg_staging_grows_with_the_batch_and_serves_groups():
    """Encode and decode one image, then five; then the five decoded with a coefficient budget of two images (groups of 2, 2, 1)."""
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    frames[:, 8:40, 8:56] //= 4          # (not noise alone: a flat region)
    sim = make()
    for n in (1, 5):
        ref = make()
        want = ref.encode_jpeg(frames[:n], 90)
        got = sim.encode_jpeg(frames[:n], 90)
        assert got == want and len(got) == n and all(len(s) > 600 for s in got)
        assert sim.decode_jpeg(got).tobytes() == ref.decode_jpeg(want).tobytes()
        ref.close()
    streams = sim.encode_jpeg(frames, 90)
    per_img = 3 * 4 * 384 * 2          # int16 coefficients of the 3 x 4 MCUs of a 48 x 64 image
    ref = make()
    want = ref.decode_jpeg(streams, upsample="triangle")
    for s in (sim, make()):          # the handle that has decoded five at once, and one whose first decode is grouped
        s.set_option("jpeg_decode_budget", 2 * per_img + 100)
        assert s.decode_jpeg(streams, upsample="triangle").tobytes() == want.tobytes()
        s.close()
    ref.close()


def test_augment_scratch_and_point_cloud_scratch_regrow():
    """avsim_image_augment with six sharpness + affine outputs through a scratch that holds two images, then through the default one (a larger
    allocation on the same handle); avsim_point_cloud with one camera, then three (longer candidate lists, more pose records)."""
    from av_aloha_amd import imgaug
    rng = np.random.default_rng(12)
    n, oh, ow = 7, 30, 40
    u8 = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    bm = np.zeros((n, 4), dtype=np.int32)
    bm[:, 0], bm[:, 1], bm[:, 2], bm[:, 3] = rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n), rng.integers(0, 64, n)
    bm[:6, 3] |= 48          # sharpness and the affine op: through the scratch images
    fac = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n), rng.uniform(0.5, 1.5, n), rng.uniform(-0.05, 0.05, n), rng.uniform(0.8, 1.2, n)], axis=1).astype(np.float32)
    mat = np.stack([imgaug.affine_matrix(rng.uniform(-20, 20), rng.integers(-6, 7), rng.integers(-2, 3), rng.uniform(0.8, 1.25)) for _ in range(n)])
    sim = make()
    for scratch in (2 * 12 * H * W + 100, 128 << 20):
        ref = make(augment_scratch_bytes=scratch)
        sim.set_option("augment_scratch_bytes", scratch)
        want = ref.augment_images(u8, (bm, fac), mat, (oh, ow), interp=1)
        assert np.isfinite(want).all() and want.std() > 0
        assert sim.augment_images(u8, (bm, fac), mat, (oh, ow), interp=1).tobytes() == want.tobytes(), scratch
        ref.close()
    bounds = (-0.6, -0.6, -0.1, 0.6, 0.6, 0.8)
    for cams in (CAMS[:1], CAMS):
        ref = make()
        want = ref.point_cloud(cams, H, W, bounds, 64)
        assert (want[2][:, 1] > 0).all()
        for a, b in zip(sim.point_cloud(cams, H, W, bounds, 64), want):
            assert a.tobytes() == b.tobytes(), cams
        ref.close()
    sim.close()


def test_set_up_twice_on_one_handle():
    """avsim_chunk_setup, avsim_obs_history_setup and avsim_episode_setup with a larger, then a smaller size: the second set-up frees the first
    one's arrays and the handle then computes what a handle that was set up once computes."""
    from av_aloha_amd.vec_env import OBJECT_BOXES
    rng = np.random.default_rng(13)
    sim, ref = make(), make()
    nj = sim.nj
    eid = np.arange(N, dtype=np.int64)
    # action chunks, temporal ensembling: C = 8, then 4
    sim.chunk_setup(8, ensemble=0.01)
    sim.chunk_step(rng.standard_normal((N, 8, nj)).astype(np.float32), eid, np.zeros(N, np.int32))
    for s in (sim, ref):
        s.chunk_setup(4, ensemble=0.01)
    for t in range(3):
        chunks = rng.standard_normal((N, 4, nj)).astype(np.float32)
        want = ref.chunk_step(chunks, eid, np.full(N, t, np.int32))
        assert want.std() > 0 and sim.chunk_step(chunks, eid, np.full(N, t, np.int32)).tobytes() == want.tobytes(), t
    # observation histories of the joints: K = 4, then 2
    sim.obs_history_setup(4)
    sim.obs_history_push(rng.standard_normal((N, nj)).astype(np.float32), None, eid, np.zeros(N, np.int32))
    for s in (sim, ref):
        s.obs_history_setup(2)
    for t in range(3):
        st = rng.standard_normal((N, nj)).astype(np.float32)
        want = ref.obs_history_push(st, None, eid, np.full(N, t, np.int32))[0]
        assert np.isfinite(want).all() and sim.obs_history_push(st, None, eid, np.full(N, t, np.int32))[0].tobytes() == want.tobytes(), t
    # episodes: a log of 8 records, then of 2
    box, share = np.ascontiguousarray(OBJECT_BOXES[TASK][0], dtype=np.float64), np.ascontiguousarray(OBJECT_BOXES[TASK][1], dtype=np.int32)

    def ep_setup(s, log):
        s.h.check(s.h.L.avsim_episode_setup(s.h.h, box.ctypes.data, share.ctypes.data, 1234, 50, 1, log))

    def ep_step(s, action):
        ap, rw, su = np.empty((N, nj)), np.empty(N, np.int32), np.empty(N, np.uint8)
        te, tr, ids, el = np.empty(N, np.uint8), np.empty(N, np.uint8), np.empty(N, np.int64), np.empty(N, np.int32)
        s.h.check(s.h.L.avsim_episode_step(s.h.h, action.ctypes.data, 10, *(a.ctypes.data for a in (ap, rw, su, te, tr, ids, el))))
        return b"".join(a.tobytes() for a in (ap, rw, su, te, tr, ids, el)) + state_bytes(s)
    home = ref.step_ctrl()[0].astype(np.float32)          # the joint positions as the action: the arms hold their pose
    ep_setup(sim, 8)
    ep_step(sim, home)
    sim.set_state(*ref.get_state())          # (the first set-up's episode moved the envs: both handles from one state again)
    sim.set_latch(ref.get_latch())
    for s in (sim, ref):
        ep_setup(s, 2)
    for t in range(3):
        a = home + np.float32(0.01) * rng.standard_normal((N, nj)).astype(np.float32)
        assert ep_step(sim, a) == ep_step(ref, a), t
    sim.close()
    ref.close()


def test_contact_capacities_raised_and_lowered_back():
    """Options "maxcon" / "maxefc" raised, then back at their first values (every contact buffer reallocated twice, the second time smaller), then 20
    steps: the state equals, bit for bit, that of a handle that was given the final values alone."""
    sim, ref = make(), make()
    con, efc = sim.maxcon, sim.maxefc
    sim.set_option("maxcon", con + 24)
    sim.set_option("maxefc", efc + 96)
    sim.step_ctrl()
    sim.set_state(*ref.get_state())
    sim.set_latch(ref.get_latch())
    for s in (sim, ref):
        s.set_option("maxcon", con)
        s.set_option("maxefc", efc)
    assert (sim.maxcon, sim.maxefc) == (con, efc)
    for _ in range(20):
        a, b = sim.step_ctrl(), ref.step_ctrl()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert state_bytes(sim) == state_bytes(ref)
    nc, pairs, dist = sim.contacts()
    rc, rpairs, rdist = ref.contacts()
    assert nc.sum() > 0 and nc.tobytes() == rc.tobytes() and pairs.tobytes() == rpairs.tobytes() and dist.tobytes() == rdist.tobytes()
    sim.close()
    ref.close()


def test_kernel_timers_count_every_launch_across_a_fold():
    """Option "kernel_timing": EV_RING + 6 single-substep steps of 2 envs -- the event list is folded into the running sum once on the way -- are that
    many launches, their time is above zero and not above the wall time of the loop, and a read with reset leaves 0 and 0.  The same for the depth
    renderer's timer over 5 renders."""
    sim = make(2, kernel_timing=1)
    L, h = sim.h.L, sim.h.h

    def read(fn, reset):
        ms, n = C.c_double(-1), C.c_int64(-1)
        sim.h.check(fn(h, reset, C.byref(ms), C.byref(n)))
        return ms.value, n.value
    read(L.avsim_kernel_time, 1)          # (make()'s own steps)
    assert read(L.avsim_kernel_time, 0) == (0.0, 0)

    def timed(fn, count, call):
        sim.h.check(L.avsim_sync(h))
        t0 = time.perf_counter()
        for _ in range(count):
            call()
        sim.h.check(L.avsim_sync(h))
        wall_ms = 1e3 * (time.perf_counter() - t0)
        ms, n = read(fn, 0)
        print(f"{fn.__name__}: {n} launches, {ms:.3f} ms of kernels in {wall_ms:.3f} ms")
        assert n == count and 0 < ms <= wall_ms
        assert read(fn, 1) == (ms, n)          # (the same figures once more, then gone)
        assert read(fn, 0) == (0.0, 0)
    timed(L.avsim_kernel_time, EV_RING + 6, lambda: sim.step_ctrl(nsub=1))
    timed(L.avsim_render_kernel_time, 5, lambda: sim.render_depth(CAMS[:2], H, W))
    sim.close()
