"""avsim_voxel_grid on the device (csrc/avsim_pointcloud.hip, the k_vox_* kernels) against its specification (av_aloha_amd/voxel.py): bit for
bit given the poses read back through avsim_camera_poses, through a host-pointer handle and through a device handle with a sentinel guard
region round `out`, with and without a colour image; against avsim_point_cloud of the same depth, without the specification; and the
vector env's observation.  slot_insertion, 3 arms, N = 3 in the three arm configurations of test_gpu_pointcloud.py."""
import numpy as np
import pytest

from av_aloha_amd import pointcloud as pc
from av_aloha_amd import voxel
from gpu_util import Guarded, torch as T
from test_gpu_pointcloud import CAMS2, FAR, N, SENTINEL, WIDE, ids_of, noise_depth, noise_rgb
from test_gpu_pointcloud import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

GUARD = 1024            # int32 words before `out`: a multiple of 4, the call wants 16-byte alignment
BOX = np.array([-2.0, -2.0, -1.5, 2.0, 2.0, 2.5], dtype=np.float32)


def grid_on_device(dev, ids, H, W, depth, rgb, bounds, max_depth, grid, null=None, ncam=None, size_grid=None, offset=0):
    """avsim_voxel_grid into the middle of a sentinel-filled tensor -> (rc, out [N, gx, gy, gz, 8], no word around it was written, the raw
    body)."""
    g = np.ascontiguousarray(grid, dtype=np.int32)
    sg = g if size_grid is None else np.asarray(size_grid)
    buf = Guarded(dev.d, N * int(sg[0]) * int(sg[1]) * int(sg[2]) * 8, T.int32, SENTINEL, GUARD, 1024)
    t_depth = T.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(dev.d)
    t_rgb = None if rgb is None else T.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(dev.d)
    bounds = np.ascontiguousarray(bounds, dtype=np.float32)
    args = {"cam_ids": ids.ctypes.data, "depth": t_depth.data_ptr(), "bounds": bounds.ctypes.data, "grid": g.ctypes.data, "out": buf.ptr(offset)}
    if null:
        args[null] = None
    rc = dev.h.L.avsim_voxel_grid(dev.h.h, args["cam_ids"], len(ids) if ncam is None else ncam, H, W, args["depth"], None if t_rgb is None else t_rgb.data_ptr(),
                                  args["bounds"], float(max_depth), args["grid"], args["out"])
    T.cuda.synchronize()
    body, intact, _ = buf.read()
    return rc, body.view(np.float32).reshape(N, int(sg[0]), int(sg[1]), int(sg[2]), 8), intact, body


def same(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert len(bad) == 0, f"{what}: differs at {bad[:4].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r} ({len(bad)} values)"


def both_equal_the_reference(sim, dev, cams, H, W, depth, rgb, bounds, max_depth, grid, what):
    """The host-pointer handle and the device handle against the specification under their own poses, with the colour image (when there is
    one) and without -> the specification's result with it."""
    ids = ids_of(sim, cams)
    poses, dposes = sim.camera_poses(cams), dev.poses(ids)
    want = None
    for colour in ([rgb, None] if rgb is not None else [None]):
        tag = f"{what}, {'with' if colour is not None else 'without'} colour"
        w = voxel.voxel_grid_reference(poses, depth, colour, bounds, max_depth, grid)
        same(sim.voxel_grid(cams, H, W, bounds, grid, max_depth=max_depth, depth=depth, rgb=colour), w, tag + ", host pointers")
        dw = w if np.array_equal(dposes, poses) else voxel.voxel_grid_reference(dposes, depth, colour, bounds, max_depth, grid)
        rc, out, intact, _ = grid_on_device(dev, ids, H, W, depth, colour, bounds, max_depth, voxel.grid_dims(grid))
        assert rc == 0, dev.h.L.avsim_last_error(dev.h.h)
        same(out, dw, tag + ", device pointers")
        assert intact, tag + ": a write outside out"
        want = w if want is None else want
    return want


def base_case(sim):
    """Noise in [0.3, 1.5] with a third of the pixels at the far plane; the box ends at the x median of env 0's valid points (the
    specification's own world points); env 1 has no candidate."""
    H, W = 24, 32
    poses = sim.camera_poses(CAMS2)
    depth = noise_depth(21, 2, H, W)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    bounds = BOX.copy()
    bounds[3] = np.median(w0[depth[0].reshape(-1) < FAR, 0])
    depth[1] = FAR
    return H, W, depth, noise_rgb(22, 2, H, W), bounds


@pytest.mark.parametrize("grid", [(8, 8, 8), (5, 7, 3)])
def test_base_case(sim, dev, grid):
    H, W, depth, rgb, bounds = base_case(sim)
    want = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, rgb, bounds, FAR, grid, f"base case, grid {grid}")
    valid0 = int((depth[0] < FAR).sum())
    assert 0.2 * valid0 < want[0, ..., 6].sum() < 0.65 * valid0          # about half of env 0's valid points, less what the box drops on y and z
    assert not want[1].any() and want[2, ..., 7].sum() > 1
    occ = want[..., 7] == 1
    assert ((want[..., 6] > 0) == occ).all() and not want[~occ].any()
    assert want[occ][:, 3:6].min() >= 0 and want[occ][:, 3:6].max() <= 1 and want[occ][:, 3:6].max() > 0.3
    lo, hi = bounds[:3], bounds[3:]
    assert (want[occ][:, :3] >= lo).all() and (want[occ][:, :3] <= hi).all()


def test_one_cell_takes_every_pixel(sim, dev):
    """Constant depth and grid (1, 1, 1): every lane of every wave adds into one cell -- the contention, and runs as long as a wave."""
    H, W = 24, 32
    depth = np.full((N, 2, H, W), 0.8, dtype=np.float32)
    want = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, noise_rgb(23, 2, H, W), WIDE, FAR, 1, "one cell")
    assert want.shape == (N, 1, 1, 1, 8) and (want[..., 6] == 2 * H * W).all() and (want[..., 7] == 1).all()


@pytest.mark.parametrize("H,W", [(7, 9), (5, 13), (1, 1)])
def test_small_images(sim, dev, H, W):
    """63 and 65 pixels: a partial wave, and a run across a wave's end; and one pixel."""
    depth = noise_depth(24 + H, 1, H, W, far_share=0.0)
    want = both_equal_the_reference(sim, dev, ["wrist_cam_left"], H, W, depth, noise_rgb(25, 1, H, W), WIDE, FAR, (2, 2, 2), f"{H} x {W}")
    assert (want[..., 6].reshape(N, -1).sum(1) == H * W).all()


@pytest.mark.parametrize("grid", [(256, 1, 1), (1, 1, 256)])
def test_grids_at_their_extents(sim, dev, grid):
    H, W = 24, 32
    depth = noise_depth(26, 2, H, W)
    want = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, noise_rgb(27, 2, H, W), BOX, FAR, grid, f"grid {grid}")
    assert (want[..., 7].reshape(N, -1).sum(1) > 8).all()


def test_runs_of_length_one(sim, dev):
    """A 1 x 64 image whose depth alternates from lane to lane between a near and a far value -- the nearest (even columns) or the farthest
    (odd columns) of 13 depths in [0.3, 1.5] that keeps the pixel inside the box and out of its left neighbour's cell; a one-row image is
    very wide -- so that no two neighbours fall in the same cell: every run has length 1."""
    H, W, grid = 1, 64, (64, 64, 64)
    depth = np.empty((N, 1, H, W), dtype=np.float32)
    poses = sim.camera_poses(["zed_cam_left"])
    for n in range(N):
        at = {}
        depths = [float(d) for d in np.linspace(0.3, 1.5, 13)]
        for d in depths:
            full = np.full((1, H, W), d, dtype=np.float32)
            world = pc.deproject(poses[n], full)
            i, _ = voxel.cells(world.reshape(-1, 3), WIDE, grid)
            inside = np.zeros(W, dtype=bool)
            inside[pc.candidates(world, full, WIDE, FAR)] = True
            at[d] = ((i[:, 0] * 64 + i[:, 1]) * 64 + i[:, 2], inside)
        last = -1
        for c in range(W):
            order = depths if c % 2 == 0 else depths[::-1]
            d = next((d for d in order if at[d][1][c] and at[d][0][c] != last), None)
            assert d is not None, "the case wants every pixel inside the box, in another cell than its left neighbour"
            depth[n, 0, 0, c], last = d, at[d][0][c]
    both_equal_the_reference(sim, dev, ["zed_cam_left"], H, W, depth, noise_rgb(28, 1, H, W), WIDE, FAR, grid, "runs of length 1")


def test_calls_in_a_row_with_the_host_arrays_overwritten(sim, dev):
    """Four device-mode calls without a synchronisation between them; bounds, camera ids and grid dims are overwritten as soon as a call
    returns: the call took them by value."""
    H, W = 24, 32
    ids = ids_of(sim, CAMS2)
    poses = dev.poses(ids)
    depth, rgb = noise_depth(29, 2, H, W), noise_rgb(30, 2, H, W)
    t_depth, t_rgb = T.from_numpy(depth).to(dev.d), T.from_numpy(rgb).to(dev.d)
    bounds, cam, g = np.zeros(6, dtype=np.float32), np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    inside0 = np.zeros(len(w0), dtype=bool)
    inside0[pc.candidates(w0, depth[0], BOX, FAR)] = True
    outs, wants = [], []
    for k in range(4):
        bounds[:] = BOX
        bounds[3 + k % 3] = np.quantile(w0[:, k % 3][inside0], 0.3 + 0.15 * k)
        cam[:] = ids
        g[:] = (4 + k, 6, 3 + 2 * k)
        wants.append(voxel.voxel_grid_reference(poses, depth, rgb, bounds.copy(), FAR, tuple(g)))
        o = T.empty((N, int(g[0]), int(g[1]), int(g[2]), 8), dtype=T.float32, device=dev.d)
        dev.h.check(dev.h.L.avsim_voxel_grid(dev.h.h, cam.ctypes.data, 2, H, W, t_depth.data_ptr(), t_rgb.data_ptr(), bounds.ctypes.data, float(FAR), g.ctypes.data, o.data_ptr()))
        bounds[:], cam[:], g[:] = 0, 5, 1
        outs.append(o)
    T.cuda.synchronize()
    for k in range(4):
        same(outs[k].cpu().numpy(), wants[k], f"call {k}")
    assert len({float(w[0, ..., 6].sum()) for w in wants}) == 4            # four different crops of env 0


def test_the_same_call_twice_gives_the_same_bits(sim, dev):
    H, W, depth, rgb, bounds = base_case(sim)
    ids = ids_of(sim, CAMS2)
    a = grid_on_device(dev, ids, H, W, depth, rgb, bounds, FAR, (8, 8, 8))
    b = grid_on_device(dev, ids, H, W, depth, rgb, bounds, FAR, (8, 8, 8))
    assert a[0] == 0 and b[0] == 0 and a[3].tobytes() == b[3].tobytes() and a[1][..., 7].sum() > 10
    x, y = sim.voxel_grid(CAMS2, H, W, bounds, 8, depth=depth, rgb=rgb), sim.voxel_grid(CAMS2, H, W, bounds, (8, 8, 8), depth=depth, rgb=rgb)
    assert x.tobytes() == y.tobytes()


def test_refusals_leave_out_untouched(sim, dev):
    H, W, grid = 24, 32, (4, 5, 6)
    ids = ids_of(sim, CAMS2)
    depth = noise_depth(31, 2, H, W)
    nan, inf = float("nan"), float("inf")
    b = lambda k, v: [v if i == k else x for i, x in enumerate(BOX.tolist())]
    cases = [("height 0", dict(H=0)), ("width 65536", dict(W=65536)), ("height -1", dict(H=-1)), ("a NaN bound", dict(bounds=b(1, nan))),
             ("an infinite bound", dict(bounds=b(4, inf))), ("lo > hi", dict(bounds=b(2, 60.0))), ("lo == hi", dict(bounds=b(0, 2.0))),
             ("max_depth 0", dict(max_depth=0.0)), ("max_depth -1", dict(max_depth=-1.0)), ("max_depth inf", dict(max_depth=inf)), ("max_depth NaN", dict(max_depth=nan)),
             ("a camera id too large", dict(ids=np.array([0, len(dev.names)], dtype=np.int32))), ("a negative camera id", dict(ids=np.array([-1, 0], dtype=np.int32))),
             ("ncam 0", dict(ncam=0)), ("ncam 17", dict(ncam=17)), ("more than 2^24 pixels", dict(H=4097, W=2048)),
             ("a grid dim 0", dict(grid=(4, 0, 6))), ("a grid dim 257", dict(grid=(257, 1, 1))), ("a negative grid dim", dict(grid=(4, 5, -6))),
             ("more than 2^21 cells", dict(grid=(129, 128, 128))), ("out not 16-byte aligned", dict(offset=4))]
    cases += [(f"{name} NULL", dict(null=name)) for name in ("cam_ids", "depth", "bounds", "grid", "out")]
    for what, kw in cases:
        a = dict(ids=ids, H=H, W=W, depth=depth, bounds=BOX, max_depth=FAR, grid=grid)
        a.update({k: v for k, v in kw.items() if k in a})
        rc, _, intact, body = grid_on_device(dev, a["ids"], a["H"], a["W"], a["depth"], None, a["bounds"], a["max_depth"], a["grid"], null=kw.get("null"), ncam=kw.get("ncam"),
                                             size_grid=grid, offset=kw.get("offset", 0))
        assert rc == -1, f"{what}: rc {rc}"
        assert intact and (body == SENTINEL).all(), f"{what}: out was written"
        assert dev.h.L.avsim_last_error(dev.h.h)
        if "null" in kw or "ncam" in kw or "offset" in kw or kw.get("H") == 4097:
            continue
        with pytest.raises(ValueError):          # the numpy layer: the library's refusal, and the specification's own check
            sim.voxel_grid(CAMS2 if "ids" not in kw else [int(x) for x in kw["ids"]], a["H"], a["W"], a["bounds"], a["grid"], max_depth=a["max_depth"],
                           depth=np.zeros((N, 2, max(a["H"], 0), max(a["W"], 0)), dtype=np.float32) if (a["H"], a["W"]) != (H, W) else depth)
        with pytest.raises(ValueError):
            voxel.check_voxel_grid(len(dev.names), a["ids"], a["H"], a["W"], a["bounds"], a["max_depth"], a["grid"])
    # the limits themselves pass, and after all that the next good call is right
    voxel.check_voxel_grid(len(dev.names), ids, H, W, BOX, FAR, (128, 128, 128))
    both_equal_the_reference(sim, dev, CAMS2, H, W, depth, None, BOX, FAR, grid, "after the refusals")


def test_more_envs_than_a_chunk():
    """1027 envs go through the kernels as a chunk of 1024 and one of 3: depth, colour and out of the second chunk start at their own
    offsets.  One camera, 5 x 6, another depth image per env."""
    from av_aloha_amd.sim import BatchedSim
    from test_oracle_physics import OBJ
    n, H, W, grid = 1027, 5, 6, (3, 2, 4)
    s = BatchedSim("slot_insertion", 3, n)
    try:
        s.reset(np.repeat(OBJ[None], n, 0))
        rng = np.random.default_rng(33)
        depth = rng.uniform(0.3, 1.5, (n, 1, H, W)).astype(np.float32)
        rgb = rng.integers(0, 256, (n, 1, H, W, 3), dtype=np.uint8)
        poses = s.camera_poses(["wrist_cam_right"])
        got = s.voxel_grid(["wrist_cam_right"], H, W, BOX, grid, depth=depth, rgb=rgb)
        want = voxel.voxel_grid_reference(poses, depth, rgb, BOX, FAR, grid)
        assert got.shape == (n, 3, 2, 4, 8) and got.view(np.int32).tobytes() == want.view(np.int32).tobytes()
        assert want[1024:, ..., 6].sum() > 30 and not np.array_equal(want[1024], want[0])
    finally:
        s.close()


# ---- against avsim_point_cloud: no specification below this line ----------------------------------------------------------------------

def test_grid_and_point_cloud_agree(sim):
    """Every point avsim_point_cloud returns for the same depth, cameras and box lies in a cell whose occupancy is 1 and whose count is at
    least 1 -- the cell worked out in float64, and a point within 1e-4 of a cell (of a face) may sit on either side --, and the counts of
    the grid sum to the cloud's number of candidates."""
    H, W, g = 24, 32, np.array([6, 7, 5])
    depth = noise_depth(32, 2, H, W)
    xyz, index, count = sim.point_cloud(CAMS2, H, W, BOX, 256, depth=depth)
    out = sim.voxel_grid(CAMS2, H, W, BOX, tuple(g), depth=depth)
    assert (count[:, 0] > 100).all()
    assert np.array_equal(out[..., 6].reshape(N, -1).sum(1).astype(np.int64), count[:, 0].astype(np.int64))
    lo, hi = BOX[:3].astype(np.float64), BOX[3:].astype(np.float64)
    for n in range(N):
        u = (xyz[n, :count[n, 1]].astype(np.float64) - lo) / (hi - lo) * g
        a, b = np.clip(np.floor(u - 1e-4), 0, g - 1).astype(int), np.clip(np.floor(u + 1e-4), 0, g - 1).astype(int)
        hit = np.zeros(len(u), dtype=bool)
        for k in range(8):
            c = np.where([k & 1, k & 2, k & 4], b, a)
            hit |= (out[n, c[:, 0], c[:, 1], c[:, 2], 7] == 1) & (out[n, c[:, 0], c[:, 1], c[:, 2], 6] >= 1)
        assert hit.all(), f"env {n}: {int((~hit).sum())} cloud points in empty cells"


# ---- the layers above -------------------------------------------------------------------------------------------------------------------

SLOT = "gym_guided_vision/SlotInsertion-3Arms-v0"
VXARG = {"cameras": ["zed_cam_left", "wrist_cam_left"], "height": 24, "width": 32, "bounds": (-1.0, -1.0, -0.05, 1.0, 1.0, 1.5), "grid": (6, 5, 4), "colour": True}


def test_vector_env_observation():
    from av_aloha_amd.vec_env import make_vec
    class Recorded:
        """The library with the names of the entry points that are looked up on it."""

        def __init__(self, L):
            self.L, self.names = L, []

        def __getattr__(self, name):
            self.names.append(name)
            return getattr(self.L, name)

    def one_reset_and_step(env):
        env.L = Recorded(env.L)
        env.reset()
        env.step(env._ap.float().clone())
        names, env.L = env.L.names, env.L.L
        return names

    plain = make_vec(SLOT, 4, 3, cameras=[], seed=2)
    keys0, info0 = set(plain.reset()[0]), set(plain.reset()[1])
    calls0 = one_reset_and_step(plain)
    assert plain._vox is None and not any("voxel" in k for k in keys0) and "avsim_voxel_grid" not in calls0 and not any("render" in c for c in calls0)
    plain.close()
    for fmt, key in (("lerobot", "observation.voxels"), ("gym", "voxels")):
        env = make_vec(SLOT, 4, 3, cameras=[], seed=2, obs_format=fmt, voxels=VXARG)
        calls = one_reset_and_step(env)
        assert calls.count("avsim_voxel_grid") == 2 and [c for c in calls if c not in ("avsim_render_depth", "avsim_render_rgb", "avsim_voxel_grid")] == calls0
        obs, info = env.reset()
        if fmt == "lerobot":
            assert set(obs) == keys0 | {key} and set(info) == info0
        x = obs[key]
        assert x.dtype == T.float32 and tuple(x.shape) == (4, 8, 6, 5, 4) and x.device == env.device
        assert x.stride() == (960, 1, 160, 32, 8) and x.is_contiguous(memory_format=T.channels_last_3d)
        a = env._ap.float().clone()
        a[:, 0] += 0.2
        a[:, 14] += 0.2
        last = None
        for t in range(1, 5):
            obs, r, te, tr, info = env.step(a)
            want = env.voxel_grid(VXARG["cameras"], 24, 32, VXARG["bounds"], VXARG["grid"], colour=True, channels_first=True)
            assert tuple(want.shape) == (4, 8, 6, 5, 4) and want.stride() == obs[key].stride() and T.equal(obs[key], want), (fmt, t)
            assert (obs[key][:, 7].sum((1, 2, 3)) > 3).all() and obs[key][:, 3:6].max() > 0
            if t == 3:
                assert tr.all()
                last = obs[key].clone()
            if t == 4:          # NEXT_STEP autoreset: the new episode's first grid, not the old episode's last
                assert (info["elapsed_steps"] == 0).all() and not T.equal(obs[key], last)
        env.close()
    with pytest.raises(ValueError):
        make_vec(SLOT, 2, 3, cameras=[], voxels=VXARG, options={"render_cam_major": 1})
    with pytest.raises(ValueError):
        make_vec(SLOT, 2, 3, cameras=["zed_cam_left"], voxels=VXARG)


def test_on_demand_colour_in_an_env_that_renders_camera_major():
    """A VecEnv with `cameras` keeps "render_cam_major" on (every camera's batch contiguous).  voxel_grid(colour=True) on such an env renders
    its colour env-major all the same: the grid equals the one from an rgb put together camera by camera (with one camera the two layouts
    are one), it differs from the grid of the camera-major buffer read as env-major, and the env's own images come out as before."""
    from av_aloha_amd.vec_env import make_vec
    cams, H, W, n = ["zed_cam_left", "wrist_cam_left"], 24, 32, 3
    env = make_vec(SLOT, n, 5, cameras=cams, obs_format="gym", observation_height=H, observation_width=W, seed=4)
    try:
        obs, _ = env.reset()
        before = {c: obs["pixels"][c].clone() for c in cams}
        ids = np.array([env.manifest["camera_names"].index(c) for c in cams], dtype=np.int32)
        depth = T.empty((n, 2, H, W), dtype=T.float32, device=env.device)
        env.h.check(env.L.avsim_render_depth(env.h.h, ids.ctypes.data, 2, H, W, depth.data_ptr()))
        one = [T.empty((n, 1, H, W, 3), dtype=T.uint8, device=env.device) for _ in cams]
        for k in range(2):
            env.h.check(env.L.avsim_render_rgb(env.h.h, ids[k:k + 1].ctypes.data, 1, H, W, one[k].data_ptr()))
        rgb = T.cat(one, dim=1).contiguous()
        cam_major = T.empty((2, n, H, W, 3), dtype=T.uint8, device=env.device)
        env.h.check(env.L.avsim_render_rgb(env.h.h, ids.ctypes.data, 2, H, W, cam_major.data_ptr()))
        assert T.equal(cam_major.permute(1, 0, 2, 3, 4), rgb), "the env is expected to render camera-major"
        args = (cams, H, W, VXARG["bounds"], VXARG["grid"])
        got = env.voxel_grid(*args, depth=depth, colour=True)
        want = env.voxel_grid(*args, depth=depth, rgb=rgb)
        wrong = env.voxel_grid(*args, depth=depth, rgb=cam_major.reshape(n, 2, H, W, 3))
        assert T.equal(got, want) and not T.equal(got, wrong) and got[..., 3:6].max() > 0 and (got[..., 7].sum((1, 2, 3)) > 3).all()
        assert T.equal(env.voxel_grid(*args, colour=True), got)          # (the depth rendered by the call as well)
        again = env._obs()["pixels"]
        assert all(T.equal(again[c], before[c]) for c in cams), "the env's images changed: render_cam_major was not put back"
    finally:
        env.close()
