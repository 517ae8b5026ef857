"""avsim_camera_poses and avsim_point_cloud on the device (csrc/avsim_pointcloud.hip) against their specification
(av_aloha_amd/pointcloud.py): bit for bit in xyz, index and count given the poses read back through avsim_camera_poses, in both I/O modes;
the poses themselves and the whole path from a rendered depth image against the CPU oracle, without the specification; the vector env's
observation and the replay of a recorded episode."""
import numpy as np
import pytest

from av_aloha_amd import pointcloud as pc
from av_aloha_amd.sim import BatchedSim
from gpu_util import Guarded, device_handle_in_state, torch as T
from test_oracle_physics import OBJ, model_dict

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 0x5A5A5A5A
GUARD = 1021
FAR = np.float32(pc.FAR_PLANE)
CAMS2 = ["zed_cam_left", "wrist_cam_right"]
CAMS6 = ["zed_cam_left", "zed_cam_right", "wrist_cam_left", "wrist_cam_right", "overhead_cam", "worms_eye_cam"]
WIDE = np.array([-50, -50, -50, 50, 50, 50], dtype=np.float32)


def spread_qpos(q):
    """Three different arm configurations (the active-vision arm carries the ZED pair, the wrist cameras ride the grippers)."""
    q = q.copy()
    for n in range(len(q)):
        q[n, 0] += 0.1 * n
        q[n, 1] -= 0.05 * n
        q[n, 9] += 0.07 * n
        q[n, 16] += 0.08 * n
        q[n, 19] -= 0.06 * n
    return q


@pytest.fixture(scope="module")
def sim():
    s = BatchedSim("slot_insertion", 3, N)
    s.reset(np.repeat(OBJ[None], N, 0))
    s.set_qpos(spread_qpos(s.get_state()[0]))
    yield s
    s.close()


class Dev:
    """A device-mode handle of the same model in the same state, with torch tensors for the pointers."""

    def __init__(self, qpos):
        self.h, self.d = device_handle_in_state("slot_insertion", N, np.repeat(OBJ[None], N, 0), qpos)

    def poses(self, ids):
        out = T.empty((N, len(ids), 16), dtype=T.float32, device=self.d)
        self.h.check(self.h.L.avsim_camera_poses(self.h.h, ids.ctypes.data, len(ids), out.data_ptr()))
        return out.cpu().numpy()

    def cloud(self, ids, H, W, depth, bounds, max_depth, P, size_p=None, null=None, ncam=None):
        """avsim_point_cloud into the middle of sentinel-filled tensors -> (rc, xyz, index, count, no word around them was written, the raw
        bodies in a row)."""
        sp = P if size_p is None else size_p
        bufs = [Guarded(self.d, s, T.int32, SENTINEL, GUARD, 1024) for s in (N * sp * 3, N * sp, N * 2)]
        ptrs = [b.ptr() for b in bufs]
        t_depth = depth if isinstance(depth, T.Tensor) else T.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(self.d)
        bounds = np.ascontiguousarray(bounds, dtype=np.float32)
        args = {"cam_ids": ids.ctypes.data, "depth": t_depth.data_ptr(), "bounds": bounds.ctypes.data, "xyz": ptrs[0], "index": ptrs[1], "count": ptrs[2]}
        if null:
            args[null] = None
        rc = self.h.L.avsim_point_cloud(self.h.h, args["cam_ids"], len(ids) if ncam is None else ncam, H, W, args["depth"], args["bounds"], float(max_depth), P, args["xyz"],
                                        args["index"], args["count"])
        T.cuda.synchronize()
        body, intact, _ = zip(*(b.read() for b in bufs))
        return rc, body[0].view(np.float32).reshape(N, sp, 3), body[1].reshape(N, sp), body[2].reshape(N, 2), all(intact), np.concatenate(body)


@pytest.fixture(scope="module")
def dev(sim):
    d = Dev(sim.get_state()[0])
    d.names = sim.manifest["camera_names"]
    yield d
    d.h.close()


def ids_of(sim, cams):
    return np.array([sim.manifest["camera_names"].index(c) for c in cams], dtype=np.int32)


def same(got, want, what):
    for g, w, name in zip(got, want, ("xyz", "index", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32)) if name == "xyz" else np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:4].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r} ({len(bad)} values)"


def both_equal_the_reference(sim, dev, cams, H, W, depth, bounds, max_depth, P, what):
    """The host-pointer handle and the device handle against the specification under their own poses -> the specification's result."""
    ids = ids_of(sim, cams)
    poses = sim.camera_poses(cams)
    want = pc.point_cloud_reference(poses, depth, bounds, max_depth, P)
    same(sim.point_cloud(cams, H, W, bounds, P, max_depth=max_depth, depth=depth), want, what + ", host pointers")
    dposes = dev.poses(ids)          # (the device handle's own records: the same state, so normally the same bits)
    dwant = want if np.array_equal(dposes, poses) else pc.point_cloud_reference(dposes, depth, bounds, max_depth, P)
    rc, xyz, index, count, intact, _ = dev.cloud(ids, H, W, depth, bounds, max_depth, P)
    assert rc == 0, dev.h.L.avsim_last_error(dev.h.h)
    same((xyz, index, count), dwant, what + ", device pointers")
    assert intact, what + ": a write outside the outputs"
    return want


def noise_rgb(seed, ncam, H, W):
    return np.random.default_rng(seed).integers(0, 256, (N, ncam, H, W, 3), dtype=np.uint8)


def noise_depth(seed, ncam, H, W, far_share=1 / 3):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.3, 1.5, (N, ncam, H, W)).astype(np.float32)
    d[rng.random((N, ncam, H, W)) < far_share] = FAR
    return d


def base_case(sim):
    """Noise in [0.3, 1.5] with a third of the pixels at the far plane; env 1 sees nothing, env 2 has 5 candidates; the box keeps about half
    of env 0's valid points (its x median, from the specification's own world points)."""
    H, W = 24, 32
    poses = sim.camera_poses(CAMS2)
    depth = noise_depth(11, 2, H, W)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    valid = depth[0].reshape(-1) < FAR
    bounds = WIDE.copy()
    bounds[3] = np.median(w0[valid, 0])
    depth[1] = FAR
    full2 = np.full_like(depth[2], 0.8)
    inside = pc.candidates(pc.deproject(poses[2], full2), full2, bounds, FAR)
    assert len(inside) >= 5
    keep = inside[np.linspace(0, len(inside) - 1, 5).astype(int)]
    depth[2] = FAR
    depth[2].reshape(-1)[keep] = 0.8
    return H, W, depth, bounds


@pytest.mark.parametrize("P", [16, 64])
def test_base_case(sim, dev, P):
    H, W, depth, bounds = base_case(sim)
    xyz, index, count = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, bounds, FAR, P, f"base case, P = {P}")
    valid0 = int((depth[0] < FAR).sum())
    assert 0.35 * valid0 < count[0, 0] < 0.65 * valid0 and count[0, 1] == P
    assert count[1].tolist() == [0, 0] and not xyz[1].any() and (index[1] == -1).all()
    assert count[2].tolist() == [5, 5] and len(set(index[2].tolist())) == 5 and (index[2, 5:] == index[2, 0]).all()
    assert len(set(index[0].tolist())) == P and (np.diff(np.sort(index[0])) > 0).all()


def test_the_cap(sim, dev):
    H, W = 96, 128
    depth = noise_depth(12, 2, H, W, far_share=0.0)
    _, index, count = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, WIDE, FAR, 32, "the cap")
    assert (count == [2 * H * W, 32]).all() and 2 * H * W > pc.MAX_CANDIDATES
    assert np.isin(index, pc.cap_positions(2 * H * W)).all()            # every pixel is a candidate: its position is its pixel


def test_exact_ties(sim, dev):
    H, W = 24, 32
    depth = np.full((N, 1, H, W), 0.9, dtype=np.float32)
    _, index, _ = both_equal_the_reference(sim, dev, ["overhead_cam"], H, W, depth, WIDE, FAR, 8, "exact ties")
    assert index[0, :2].tolist() == [0, H * W - 1]


def test_small_shapes(sim, dev):
    both_equal_the_reference(sim, dev, ["wrist_cam_left"], 1, 1, np.full((N, 1, 1, 1), 0.5, dtype=np.float32), WIDE, FAR, 1, "1 x 1, P = 1")
    depth = noise_depth(13, 1, 64, 64, far_share=0.0)
    _, index, count = both_equal_the_reference(sim, dev, ["zed_cam_right"], 64, 64, depth, WIDE, FAR, 4096, "P = M = 4096")
    assert (count == [4096, 4096]).all() and (np.sort(index, axis=1) == np.arange(4096)).all()


def test_calls_in_a_row_with_the_bounds_overwritten(sim, dev):
    """Four device-mode calls without a synchronisation between them; the caller's bounds and camera ids are overwritten as soon as a call
    returns: the call took them by value."""
    H, W, P = 24, 32, 16
    ids = ids_of(sim, CAMS2)
    poses = dev.poses(ids)
    depth = noise_depth(14, 2, H, W)
    t_depth = T.from_numpy(depth).to(dev.d)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    bounds, cam = np.zeros(6, dtype=np.float32), np.zeros(2, dtype=np.int32)
    outs, wants = [], []
    for k in range(4):
        bounds[:] = WIDE
        bounds[k % 3 + 3] = np.quantile(w0[:, k % 3][depth[0].reshape(-1) < FAR], 0.3 + 0.15 * k)
        cam[:] = ids
        wants.append(pc.point_cloud_reference(poses, depth, bounds.copy(), FAR, P))
        o = (T.empty((N, P, 3), dtype=T.float32, device=dev.d), T.empty((N, P), dtype=T.int32, device=dev.d), T.empty((N, 2), dtype=T.int32, device=dev.d))
        dev.h.check(dev.h.L.avsim_point_cloud(dev.h.h, cam.ctypes.data, 2, H, W, t_depth.data_ptr(), bounds.ctypes.data, float(FAR), P, o[0].data_ptr(), o[1].data_ptr(),
                                              o[2].data_ptr()))
        bounds[:], cam[:] = 0, 5
        outs.append(o)
    T.cuda.synchronize()
    for k in range(4):
        same([x.cpu().numpy() for x in outs[k]], wants[k], f"call {k}")
    assert len({w[2][0, 0] for w in wants}) == 4            # four different crops


def test_refusals_leave_the_outputs_untouched(sim, dev):
    H, W, P = 24, 32, 16
    ids = ids_of(sim, CAMS2)
    depth = noise_depth(15, 2, H, W)
    nan, inf = float("nan"), float("inf")
    b = lambda k, v: [v if i == k else x for i, x in enumerate(WIDE.tolist())]
    cases = [("npoints 0", dict(P=0)), ("npoints 4097", dict(P=4097)), ("height 0", dict(H=0)), ("width 65536", dict(W=65536)), ("height -1", dict(H=-1)),
             ("a NaN bound", dict(bounds=b(1, nan))), ("an infinite bound", dict(bounds=b(4, inf))), ("lo > hi", dict(bounds=b(2, 60.0))),
             ("max_depth 0", dict(max_depth=0.0)), ("max_depth -1", dict(max_depth=-1.0)), ("max_depth inf", dict(max_depth=inf)), ("max_depth NaN", dict(max_depth=nan)),
             ("a camera id too large", dict(ids=np.array([0, len(dev.names)], dtype=np.int32))), ("a negative camera id", dict(ids=np.array([-1, 0], dtype=np.int32))),
             ("ncam 0", dict(ncam=0)), ("ncam 17", dict(ncam=17)), ("more than 2^24 pixels", dict(H=4097, W=2048))]
    cases += [(f"{name} NULL", dict(null=name)) for name in ("cam_ids", "depth", "bounds", "xyz", "index", "count")]
    for what, kw in cases:
        a = dict(ids=ids, H=H, W=W, depth=depth, bounds=WIDE, max_depth=FAR, P=P)
        a.update({k: v for k, v in kw.items() if k in a})
        rc, _, _, _, intact, body = dev.cloud(a["ids"], a["H"], a["W"], a["depth"], a["bounds"], a["max_depth"], a["P"], size_p=P, null=kw.get("null"), ncam=kw.get("ncam"))
        assert rc == -1, f"{what}: rc {rc}"
        assert intact and (body == SENTINEL).all(), f"{what}: the outputs were written"
        assert dev.h.L.avsim_last_error(dev.h.h)
        if "null" in kw or "ncam" in kw or kw.get("H") == 4097:
            continue
        with pytest.raises(ValueError):          # the numpy layer: the library's refusal, and the specification's own check
            sim.point_cloud(["zed_cam_left", "wrist_cam_right"] if "ids" not in kw else [int(x) for x in kw["ids"]], a["H"], a["W"], a["bounds"], a["P"], max_depth=a["max_depth"],
                            depth=np.zeros((N, 2, max(a["H"], 0), max(a["W"], 0)), dtype=np.float32) if (a["H"], a["W"]) != (H, W) else depth)
        with pytest.raises(ValueError):
            pc.check_point_cloud(len(dev.names), a["ids"], a["H"], a["W"], a["bounds"], a["max_depth"], a["P"])
    out = T.full((N * 2 * 16 + 8,), 7.0, dtype=T.float32, device=dev.d)
    for cam, ncam in ((np.array([0, 99], dtype=np.int32), 2), (ids, 0), (ids, 17)):
        assert dev.h.L.avsim_camera_poses(dev.h.h, cam.ctypes.data, ncam, out.data_ptr()) == -1
    assert dev.h.L.avsim_camera_poses(dev.h.h, None, 2, out.data_ptr()) == -1 and dev.h.L.avsim_camera_poses(dev.h.h, ids.ctypes.data, 2, None) == -1
    T.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(ValueError):
        sim.camera_poses([99])
    # and after all that the next good call is right
    both_equal_the_reference(sim, dev, CAMS2, H, W, depth, WIDE, FAR, P, "after the refusals")


# ---- against the oracle: no specification below this line ------------------------------------------------------------------------------

def quat2mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


@pytest.fixture(scope="module")
def moved():
    """The state of test_gpu_render.py::test_depth_matches_oracle_after_motion: f64 physics, solver 1, six wiggle steps, device and oracle."""
    from orc_env import OrcEnv
    from test_gpu_physics import actions_wiggle
    md = model_dict()
    s = BatchedSim("slot_insertion", 3, N, f64=True, options={"solver": 1})
    e = OrcEnv()
    e.d.solver = 1
    s.reset(np.repeat(OBJ[None], N, 0))
    e.reset(OBJ)
    for a in actions_wiggle(md, 6):
        s.step(np.repeat(a[None], N, 0))
        e.env_step(a)
    nb = md["nbody"]
    xpos, xmat = e.arr("xpos", 3 * nb).reshape(nb, 3).copy(), e.arr("xmat", 9 * nb).reshape(nb, 3, 3).copy()
    cams = {}
    for cam in CAMS6:
        c = e.man["camera_names"].index(cam)
        b = int(md["cam_body"][c])
        cams[cam] = (xpos[b] + xmat[b] @ md["cam_pos"].reshape(-1, 3)[c], xmat[b] @ quat2mat(md["cam_quat"].reshape(-1, 4)[c]),
                     np.tan(0.5 * np.deg2rad(md["cam_fovy"].reshape(-1)[c])))
    yield s, e, cams
    s.close()
    e.close()


def test_poses_against_the_oracle(moved):
    """The device's float32 pose records against float64 poses from the oracle's xpos / xmat and the blob's cam_pos / cam_quat: 1e-5 in the
    position and in every rotation entry (f64 parity is 1e-6, float32 rounding of metre-sized values over a dozen operations adds less than
    1e-6), tan(fovy / 2) within 1e-6 relative."""
    sim, e, cams = moved
    poses = sim.camera_poses(CAMS6)
    assert poses.shape == (N, 6, 16) and poses.dtype == np.float32 and not poses[:, :, 13:].any()
    assert np.array_equal(poses[0], poses[1]) and np.array_equal(poses[0], poses[2])
    dp = dr = dt = 0.0
    for ci, cam in enumerate(CAMS6):
        p, R, t = cams[cam]
        dp = max(dp, np.abs(poses[0, ci, :3] - p).max())
        dr = max(dr, np.abs(poses[0, ci, 3:12].reshape(3, 3) - R).max())
        dt = max(dt, abs(poses[0, ci, 12] / t - 1))
    print(f"camera poses against the oracle: position {dp:.3g} m, rotation entries {dr:.3g}, tan(fovy / 2) {dt:.3g} relative")
    assert dp <= 1e-5 and dr <= 1e-5 and dt <= 1e-6


def test_rendered_clouds_against_the_oracle(moved):
    """Every returned point of six single-camera clouds (60 x 80, the rendered depth, P = 256) projected into the ORACLE's camera lands within
    0.01 pixel of the centre of the pixel its index names, and its distance along the oracle's optical axis equals the oracle's depth image
    at that pixel within 1e-4 m for all but 0.5 % of the points (the depth test's tolerance and share)."""
    sim, e, cams = moved
    H, W, P = 60, 80, 256
    worst_px = worst_share = 0.0
    for cam in CAMS6:
        xyz, index, count = sim.point_cloud([cam], H, W, WIDE, P)
        ref = e.render_depth(cam, H, W)
        assert (count[:, 0] > 0).all() and (index >= 0).all() and (index < H * W).all()
        p, R, t = cams[cam]
        scale = 2.0 * t / H
        c = (xyz[0].astype(np.float64) - p) @ R             # R^T (w - p): the point in the oracle's camera frame
        z = -c[:, 2]
        assert (z > 0).all()
        col, row = c[:, 0] / z / scale + 0.5 * W, -c[:, 1] / z / scale + 0.5 * H
        r, cc = index[0] // W, index[0] % W
        worst_px = max(worst_px, np.abs(col - (cc + 0.5)).max(), np.abs(row - (r + 0.5)).max())
        bad = np.abs(z - ref[r, cc]) > 1e-4
        worst_share = max(worst_share, bad.mean())
        assert len(set(index[0].tolist())) == count[0, 1] == min(count[0, 0], P)
    print(f"rendered clouds against the oracle: {worst_px:.3g} pixel from the centre at most, {100 * worst_share:.2f} % of a cloud's points off the oracle's depth by more than 1e-4 m")
    assert worst_px <= 0.01 and worst_share <= 0.005


def test_camera_poses_through_both_fronts():
    """BatchedSim.camera_poses (numpy) and VecEnv.camera_poses (torch) are one body behind two kinds of array: two envs of insert_peg with
    different arm configurations, the same qpos in both handles -> the same bytes.  There is no numpy specification of the pose records (the
    point-cloud specification takes them from the device), so the reference is the oracle's float64 kinematics, with the bounds and the
    reasoning of test_poses_against_the_oracle: 1e-5 in the position and in every rotation entry -- the state is set, not simulated, so all
    that differs is float32 rounding of metre-sized values along a chain of a dozen bodies, a few 1e-7 --, tan(fovy / 2) within 1e-6
    relative."""
    from av_aloha_amd.vec_env import make_vec
    from orc_env import OrcEnv
    obj = np.array([[0.15, 0.0, 0.01, 1, 0, 0, 0], [-0.15, 0.0, 0.021, 1, 0, 0, 0.0]])
    md = model_dict("insert_peg")
    sim = BatchedSim("insert_peg", 3, 2)
    env = make_vec("gym_guided_vision/InsertPeg-3Arms-v0", num_envs=2, max_episode_steps=5, cameras=[])
    e = OrcEnv("insert_peg")
    try:
        sim.reset(np.repeat(obj[None], 2, 0))
        q = spread_qpos(sim.get_state()[0])
        q[0, 2] += 0.11                                              # (spread_qpos leaves env 0 at home)
        sim.set_qpos(q)
        env.reset()
        t_q = T.from_numpy(np.ascontiguousarray(q)).to(env.device)
        env.h.check(env.L.avsim_set_qpos(env.h.h, t_q.data_ptr()))
        a = sim.camera_poses(CAMS6)
        t = env.camera_poses(CAMS6)
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (2, 6, 16)
        assert t.dtype == T.float32 and tuple(t.shape) == (2, 6, 16) and t.device == env.device
        assert a.tobytes() == t.cpu().numpy().tobytes()
        assert not np.array_equal(a[0], a[1]) and not a[:, :, 13:].any()
        nb = md["nbody"]
        dp = dr = dt = 0.0
        for n in range(2):
            e.reset(obj)
            e.set_qpos(q[n])
            e.L.orc_kinematics(e.dptr)
            xpos, xmat = e.arr("xpos", 3 * nb).reshape(nb, 3), e.arr("xmat", 9 * nb).reshape(nb, 3, 3)
            for ci, cam in enumerate(CAMS6):
                c = e.man["camera_names"].index(cam)
                b = int(md["cam_body"][c])
                p, R = xpos[b] + xmat[b] @ md["cam_pos"].reshape(-1, 3)[c], xmat[b] @ quat2mat(md["cam_quat"].reshape(-1, 4)[c])
                dp = max(dp, np.abs(a[n, ci, :3] - p).max())
                dr = max(dr, np.abs(a[n, ci, 3:12].reshape(3, 3) - R).max())
                dt = max(dt, abs(a[n, ci, 12] / np.tan(0.5 * np.deg2rad(md["cam_fovy"].reshape(-1)[c])) - 1))
        print(f"camera poses of both fronts against the oracle: position {dp:.3g} m, rotation entries {dr:.3g}, tan(fovy / 2) {dt:.3g} relative")
        assert dp <= 1e-5 and dr <= 1e-5 and dt <= 1e-6
    finally:
        env.close()
        sim.close()
        e.close()


# ---- the layers above ---------------------------------------------------------------------------------------------------------------------

SLOT = "gym_guided_vision/SlotInsertion-3Arms-v0"
PCARG = {"cameras": ["zed_cam_left", "wrist_cam_left"], "height": 24, "width": 32, "bounds": (-1.0, -1.0, -0.05, 1.0, 1.0, 1.5), "points": 48}


def test_vector_env_observation():
    from av_aloha_amd.vec_env import make_vec
    plain = make_vec(SLOT, 4, 3, cameras=[], seed=2)
    keys0, info0 = set(plain.reset()[0]), set(plain.reset()[1])
    plain.close()
    for fmt, key in (("lerobot", "observation.pointcloud"), ("gym", "pointcloud")):
        env = make_vec(SLOT, 4, 3, cameras=[], seed=2, obs_format=fmt, pointcloud=PCARG)
        obs, info = env.reset()
        if fmt == "lerobot":
            assert set(obs) == keys0 | {key} and set(info) == info0 | {"pointcloud_count", "pointcloud_index"}
        x, idx, cnt = obs[key], info["pointcloud_index"], info["pointcloud_count"]
        assert x.dtype == T.float32 and tuple(x.shape) == (4, 48, 3) and x.device == env.device
        assert idx.dtype == T.int32 and tuple(idx.shape) == (4, 48) and cnt.dtype == T.int32 and tuple(cnt.shape) == (4, 2)
        a = env._ap.float().clone()
        a[:, 0] += 0.2
        a[:, 14] += 0.2
        last = None
        for t in range(1, 5):
            obs, r, te, tr, info = env.step(a)
            want = env.point_cloud(PCARG["cameras"], 24, 32, PCARG["bounds"], 48)
            for g, w in zip((obs[key], info["pointcloud_index"], info["pointcloud_count"]), want):
                assert T.equal(g, w), (fmt, t)
            assert (info["pointcloud_count"][:, 1] == 48).all() and (obs[key][:, :, 2] >= -0.05).all() and (obs[key][:, :, 2] <= 1.5).all()
            if t == 3:
                assert tr.all()
                last = obs[key].clone()
            if t == 4:          # NEXT_STEP autoreset: the new episode's first cloud, not the old episode's last
                assert (info["elapsed_steps"] == 0).all() and not T.equal(obs[key], last)
        poses = env.camera_poses(PCARG["cameras"])
        assert poses.dtype == T.float32 and tuple(poses.shape) == (4, 2, 16) and poses.device == env.device
        env.close()


def test_replay_equals_point_cloud_after_set_qpos():
    from av_aloha_amd import harness
    s = BatchedSim("slot_insertion", 3, 5)
    s.reset(np.repeat(OBJ[None], 5, 0))
    q = s.get_state()[0]
    for n in range(5):
        q[n, 0] += 0.05 * n
        q[n, 17] -= 0.04 * n
    data = {"/observations/all_qpos": q}
    cams, b = ["zed_cam_left", "zed_cam_right"], (-1.0, -1.0, 0.0, 1.0, 1.0, 1.5)
    s.set_qpos(q)
    want = s.point_cloud(cams, 24, 32, b, 40)
    s.close()
    for fpb in (128, 2):          # one batch, and batches of 2 with a ragged last one
        xyz, count = harness.rerender_pointclouds(data, SLOT, cams, 24, 32, b, 40, frames_per_batch=fpb)
        assert xyz.shape == (5, 40, 3) and xyz.dtype == np.float32 and np.array_equal(xyz.view(np.int32), want[0].view(np.int32)) and np.array_equal(count, want[2])
    assert len({x.tobytes() for x in want[0]}) == 5 and (want[2][:, 1] == 40).all()
    assert harness.parse_pointcloud_option("zed_cam_left,zed_cam_right:24:32:40:-1,-1,0,1,1,1.5") == {"cameras": cams, "height": 24, "width": 32, "points": 40, "bounds": list(b)}
