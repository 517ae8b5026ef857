"""avsim_virtual_views on the device (csrc/avsim_pointcloud.hip, the k_vv_* kernels) against its specification (av_aloha_amd/virtviews.py):
bit for bit in out and index given the poses read back through avsim_camera_poses, through a host-pointer handle and through a device handle
with sentinel guard regions round both outputs, with and without a colour image; against avsim_voxel_grid and the renderers, without the
specification; and the vector env's observation.  slot_insertion, 3 arms, N = 3 in the three arm configurations of test_gpu_pointcloud.py."""
import numpy as np
import pytest

from av_aloha_amd import pointcloud as pc
from av_aloha_amd import virtviews as vv
from gpu_util import Guarded, torch as T
from test_gpu_pointcloud import CAMS2, FAR, N, SENTINEL, WIDE, ids_of, noise_depth, noise_rgb
from test_gpu_pointcloud import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

GUARD = 1024            # int32 words before the outputs: a multiple of 4, the call wants `out` 16-byte aligned
BOX = np.array([-2.0, -2.0, -1.5, 2.0, 2.0, 2.5], dtype=np.float32)
ALL = [0, 1, 2, 3, 4, 5]


def views_on_device(dev, ids, H, W, depth, rgb, bounds, max_depth, views, size, radius, null=None, ncam=None, nviews=None, room=None, offset=0):
    """avsim_virtual_views into the middle of two sentinel-filled tensors -> (rc, out [N, V, VH, VW, 8], index [N, V, VH, VW], no word
    around them was written, the raw bodies).  room: (V, VH, VW) the buffers are sized for, when the call's own are none."""
    v, sz = np.ascontiguousarray(views, dtype=np.int32), np.ascontiguousarray(size, dtype=np.int32)
    V, VH, VW = (len(v), int(sz[0]), int(sz[1])) if room is None else room
    n_idx = N * V * VH * VW
    b_out = Guarded(dev.d, 8 * n_idx, T.int32, SENTINEL, GUARD, 1024)
    b_idx = Guarded(dev.d, n_idx, T.int32, SENTINEL, GUARD, 1024)
    t_depth = T.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(dev.d)
    t_rgb = None if rgb is None else T.from_numpy(np.ascontiguousarray(rgb, dtype=np.uint8)).to(dev.d)
    bounds = np.ascontiguousarray(bounds, dtype=np.float32)
    args = {"cam_ids": ids.ctypes.data, "depth": t_depth.data_ptr(), "bounds": bounds.ctypes.data, "views": v.ctypes.data, "size": sz.ctypes.data,
            "out": b_out.ptr(offset), "index": b_idx.ptr()}
    if null:
        args[null] = None
    rc = dev.h.L.avsim_virtual_views(dev.h.h, args["cam_ids"], len(ids) if ncam is None else ncam, H, W, args["depth"], None if t_rgb is None else t_rgb.data_ptr(), args["bounds"],
                                     float(max_depth), args["views"], len(v) if nviews is None else nviews, args["size"], int(radius), args["out"], args["index"])
    T.cuda.synchronize()
    (body_o, intact_o, _), (body_i, intact_i, _) = b_out.read(), b_idx.read()
    return rc, body_o.view(np.float32).reshape(N, V, VH, VW, 8), body_i.reshape(N, V, VH, VW), intact_o and intact_i, (body_o, body_i)


def same(got, want, what):
    for g, w, name in zip(got, want, ("out", "index")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g.view(np.int32) != w.view(np.int32))
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:4].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r} ({len(bad)} values)"


def both_equal_the_reference(sim, dev, cams, H, W, depth, rgb, bounds, max_depth, views, size, radius, what):
    """The host-pointer handle and the device handle against the specification under their own poses, with the colour image (when there is
    one) and without -> the specification's (out, index) with it."""
    ids = ids_of(sim, cams)
    poses, dposes = sim.camera_poses(cams), dev.poses(ids)
    want = None
    for colour in ([rgb, None] if rgb is not None else [None]):
        tag = f"{what}, {'with' if colour is not None else 'without'} colour"
        w = vv.virtual_views_reference(poses, depth, colour, bounds, max_depth, views, size, radius)
        same(sim.virtual_views(cams, H, W, bounds, views, size, radius=radius, max_depth=max_depth, depth=depth, rgb=colour), w, tag + ", host pointers")
        dw = w if np.array_equal(dposes, poses) else vv.virtual_views_reference(dposes, depth, colour, bounds, max_depth, views, size, radius)
        rc, out, index, intact, _ = views_on_device(dev, ids, H, W, depth, colour, bounds, max_depth, vv.view_codes(views), vv.view_size(size), radius)
        assert rc == 0, dev.h.L.avsim_last_error(dev.h.h)
        same((out, index), dw, tag + ", device pointers")
        assert intact, tag + ": a write outside out or index"
        want = w if want is None else want
    return want


def base_case(sim):
    """Noise in [0.3, 1.5] with a third of the pixels at the far plane; the box ends at the x median of env 0's valid points (the
    specification's own world points); env 1 has no candidate."""
    H, W = 24, 32
    poses = sim.camera_poses(CAMS2)
    depth = noise_depth(41, 2, H, W)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    bounds = BOX.copy()
    bounds[3] = np.median(w0[depth[0].reshape(-1) < FAR, 0])
    depth[1] = FAR
    return H, W, depth, noise_rgb(42, 2, H, W), bounds


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("size", [(16, 16), (5, 7)])
def test_base_case(sim, dev, size, radius):
    H, W, depth, rgb, bounds = base_case(sim)
    out, index = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, rgb, bounds, FAR, ALL, size, radius, f"base case, size {size}, radius {radius}")
    hit = index >= 0
    assert hit[0].reshape(6, -1).sum(1).min() > 3 and hit[2].reshape(6, -1).sum(1).min() > 3 and not hit[1].any() and not out[1].any()
    assert ((out[..., 7] == 1) == hit).all() and set(np.unique(out[..., 7]).tolist()) == {0.0, 1.0} and not out[~hit].any()
    assert out[hit][:, :3].min() >= 0 and out[hit][:, :3].max() <= 1 and out[hit][:, :3].max() > 0.5
    ext = bounds[3:] - bounds[:3]
    for v in range(6):
        d = out[:, v, ..., 3][hit[:, v]]
        assert d.min() >= 0 and d.max() <= ext[v // 2], v
    assert (out[hit][:, 4:7] >= bounds[:3]).all() and (out[hit][:, 4:7] <= bounds[3:]).all()
    assert index[hit].max() < 2 * H * W


def test_one_pixel_takes_every_candidate(sim, dev):
    """Size (1, 1): every lane of every wave takes the minimum into one address per view -- the contention, and runs as long as a wave."""
    H, W = 24, 32
    depth = noise_depth(43, 2, H, W, far_share=0.0)
    out, index = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, noise_rgb(44, 2, H, W), WIDE, FAR, ALL, (1, 1), 1, "one pixel")
    assert out.shape == (N, 6, 1, 1, 8) and (index >= 0).all()
    flat = np.full((N, 2, H, W), 0.8, dtype=np.float32)          # and with equal depths: long runs of equal targets, many equal keys' upper halves
    both_equal_the_reference(sim, dev, CAMS2, H, W, flat, None, WIDE, FAR, [4, 5], (1, 1), 0, "one pixel, constant depth")


@pytest.mark.parametrize("H,W", [(7, 9), (5, 13), (1, 1)])
def test_small_images(sim, dev, H, W):
    """63 and 65 pixels: a partial wave, and a run across a wave's end; and one pixel."""
    depth = noise_depth(45 + H, 1, H, W, far_share=0.0)
    out, index = both_equal_the_reference(sim, dev, ["wrist_cam_left"], H, W, depth, noise_rgb(46, 1, H, W), WIDE, FAR, ALL, (4, 6), 1, f"{H} x {W}")
    assert (index >= 0).reshape(N, 6, -1).any(2).all() and index.max() < H * W


def test_every_footprint_is_clipped(sim, dev):
    """Size (3, 3) with radius 4: every footprint covers the whole image, clipped on all sides."""
    H, W = 24, 32
    depth = noise_depth(47, 2, H, W)
    out, index = both_equal_the_reference(sim, dev, CAMS2, H, W, depth, noise_rgb(48, 2, H, W), BOX, FAR, ALL, (3, 3), 4, "3 x 3, radius 4")
    for n in range(N):
        for v in range(6):
            assert len(np.unique(index[n, v])) == 1 and index[n, v, 0, 0] >= 0          # the nearest point of the env covers every pixel


def test_ties_on_the_device(sim, dev):
    """The same camera in both slots with the same depth image: every point exists twice at equal dist, and the lower slot wins."""
    H, W = 24, 32
    one = noise_depth(49, 1, H, W)
    depth = np.concatenate([one, one], axis=1)
    for cam in ("zed_cam_left", "wrist_cam_right"):
        out, index = both_equal_the_reference(sim, dev, [cam, cam], H, W, depth, noise_rgb(50, 2, H, W), BOX, FAR, ALL, (16, 16), 1, f"{cam} twice")
        assert (index >= 0).sum() > 100 and index.max() < H * W


def test_calls_in_a_row_with_the_host_arrays_overwritten(sim, dev):
    """Four device-mode calls without a synchronisation between them; bounds, camera ids, views and size are overwritten as soon as a call
    returns: the call took them by value."""
    H, W = 24, 32
    ids = ids_of(sim, CAMS2)
    poses = dev.poses(ids)
    depth, rgb = noise_depth(51, 2, H, W), noise_rgb(52, 2, H, W)
    t_depth, t_rgb = T.from_numpy(depth).to(dev.d), T.from_numpy(rgb).to(dev.d)
    bounds, cam, views, size = np.zeros(6, dtype=np.float32), np.zeros(2, dtype=np.int32), np.zeros(6, dtype=np.int32), np.zeros(2, dtype=np.int32)
    w0 = pc.deproject(poses[0], depth[0]).reshape(-1, 3)
    inside0 = np.zeros(len(w0), dtype=bool)
    inside0[pc.candidates(w0, depth[0], BOX, FAR)] = True
    outs, wants = [], []
    for k in range(4):
        bounds[:] = BOX
        bounds[3 + k % 3] = np.quantile(w0[:, k % 3][inside0], 0.3 + 0.15 * k)
        cam[:] = ids
        nv = 2 + k
        views[:nv] = [(3 * k + j) % 6 for j in range(nv)]
        size[:] = (6 + k, 9 - k)
        wants.append(vv.virtual_views_reference(poses, depth, rgb, bounds.copy(), FAR, views[:nv].copy(), tuple(size), k % 3))
        o = T.empty((N, nv, int(size[0]), int(size[1]), 8), dtype=T.float32, device=dev.d)
        i = T.empty((N, nv, int(size[0]), int(size[1])), dtype=T.int32, device=dev.d)
        dev.h.check(dev.h.L.avsim_virtual_views(dev.h.h, cam.ctypes.data, 2, H, W, t_depth.data_ptr(), t_rgb.data_ptr(), bounds.ctypes.data, float(FAR), views.ctypes.data, nv,
                                                size.ctypes.data, k % 3, o.data_ptr(), i.data_ptr()))
        bounds[:], cam[:], views[:], size[:] = 0, 5, 7, 1
        outs.append((o, i))
    T.cuda.synchronize()
    for k in range(4):
        same((outs[k][0].cpu().numpy(), outs[k][1].cpu().numpy()), wants[k], f"call {k}")
    assert all((w[1][0] >= 0).sum() > 5 for w in wants)


def test_the_same_call_twice_gives_the_same_bytes(sim, dev):
    H, W, depth, rgb, bounds = base_case(sim)
    ids = ids_of(sim, CAMS2)
    a = views_on_device(dev, ids, H, W, depth, rgb, bounds, FAR, ALL, (16, 16), 1)
    b = views_on_device(dev, ids, H, W, depth, rgb, bounds, FAR, ALL, (16, 16), 1)
    assert a[0] == 0 and b[0] == 0 and a[4][0].tobytes() == b[4][0].tobytes() and a[4][1].tobytes() == b[4][1].tobytes() and (a[2] >= 0).sum() > 100
    x = sim.virtual_views(CAMS2, H, W, bounds, ALL, 16, depth=depth, rgb=rgb)
    y = sim.virtual_views(CAMS2, H, W, bounds, list(vv.VIEW_NAMES), (16, 16), depth=depth, rgb=rgb)
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()


def test_refusals_leave_the_outputs_untouched(sim, dev):
    H, W, views, size, radius = 24, 32, [4, 0, 1], (4, 5), 1
    ids = ids_of(sim, CAMS2)
    depth = noise_depth(53, 2, H, W)
    nan, inf = float("nan"), float("inf")
    b = lambda k, v: [v if i == k else x for i, x in enumerate(BOX.tolist())]
    cases = [("height 0", dict(H=0)), ("width 65536", dict(W=65536)), ("height -1", dict(H=-1)), ("a NaN bound", dict(bounds=b(1, nan))),
             ("an infinite bound", dict(bounds=b(4, inf))), ("lo > hi", dict(bounds=b(2, 60.0))), ("lo == hi", dict(bounds=b(0, 2.0))),
             ("max_depth 0", dict(max_depth=0.0)), ("max_depth -1", dict(max_depth=-1.0)), ("max_depth inf", dict(max_depth=inf)), ("max_depth NaN", dict(max_depth=nan)),
             ("a camera id too large", dict(ids=np.array([0, len(dev.names)], dtype=np.int32))), ("a negative camera id", dict(ids=np.array([-1, 0], dtype=np.int32))),
             ("ncam 0", dict(ncam=0)), ("ncam 17", dict(ncam=17)), ("more than 2^24 pixels", dict(H=4097, W=2048)),
             ("nviews 0", dict(nviews=0)), ("nviews 7", dict(nviews=7)), ("nviews -1", dict(nviews=-1)), ("a view code 6", dict(views=[4, 6, 1])), ("a view code -1", dict(views=[-1, 0, 1])),
             ("a size 0", dict(size=(0, 5))), ("a size 1025", dict(size=(4, 1025))), ("a negative size", dict(size=(-4, 5))),
             ("radius -1", dict(radius=-1)), ("radius 5", dict(radius=5)),
             ("an extent whose inv is not finite", dict(bounds=[0, 0, 0, 1, 1, 1e-37], size=(1024, 5))), ("an extent that is not finite", dict(bounds=[-3e38, 0, 0, 3e38, 1, 1])),
             ("out not 16-byte aligned", dict(offset=4)), ("out 8-byte aligned", dict(offset=8))]
    cases += [(f"{name} NULL", dict(null=name)) for name in ("cam_ids", "depth", "bounds", "views", "size", "out", "index")]
    for what, kw in cases:
        a = dict(ids=ids, H=H, W=W, depth=depth, bounds=BOX, max_depth=FAR, views=views, size=size, radius=radius)
        a.update({k: v for k, v in kw.items() if k in a})
        rc, _, _, intact, body = views_on_device(dev, a["ids"], a["H"], a["W"], a["depth"], None, a["bounds"], a["max_depth"], a["views"], a["size"], a["radius"], null=kw.get("null"),
                                                 ncam=kw.get("ncam"), nviews=kw.get("nviews"), room=(3, 4, 5), offset=kw.get("offset", 0))
        assert rc == -1, f"{what}: rc {rc}"
        assert intact and (body[0] == SENTINEL).all() and (body[1] == SENTINEL).all(), f"{what}: an output was written"
        assert dev.h.L.avsim_last_error(dev.h.h)
        if "null" in kw or "ncam" in kw or "nviews" in kw or "offset" in kw or kw.get("H") == 4097:
            continue
        with pytest.raises(ValueError):          # the numpy layer: the library's refusal, or the front's own before it
            sim.virtual_views(CAMS2 if "ids" not in kw else [int(x) for x in kw["ids"]], a["H"], a["W"], a["bounds"], a["views"], a["size"], radius=a["radius"], max_depth=a["max_depth"],
                              depth=np.zeros((N, 2, max(a["H"], 0), max(a["W"], 0)), dtype=np.float32) if (a["H"], a["W"]) != (H, W) else depth)
        with pytest.raises(ValueError):
            vv.check_virtual_views(len(dev.names), a["ids"], a["H"], a["W"], a["bounds"], a["max_depth"], a["views"], a["size"], a["radius"])
    for views7 in ([], [0] * 7):          # the number of views, through the layers that take a list
        with pytest.raises(ValueError):
            sim.virtual_views(CAMS2, H, W, BOX, views7, size, depth=depth)
        with pytest.raises(ValueError):
            vv.check_virtual_views(len(dev.names), ids, H, W, BOX, FAR, views7, size, radius)
    # the limits themselves pass: size 1024, radius 4, six views (one camera of 2 x 2 keeps it small); and after all that the next good call is right
    vv.check_virtual_views(len(dev.names), ids, H, W, BOX, FAR, ALL, (1024, 1024), 4)
    small = noise_depth(54, 1, 2, 2, far_share=0.0)
    got = sim.virtual_views(["zed_cam_left"], 2, 2, BOX, ALL, (1024, 1), radius=4, depth=small)
    same(got, vv.virtual_views_reference(sim.camera_poses(["zed_cam_left"]), small, None, BOX, FAR, ALL, (1024, 1), 4), "six views of 1024 x 1, radius 4")
    got = sim.virtual_views(["zed_cam_left"], 2, 2, BOX, [4], (2, 1024), radius=4, depth=small)
    same(got, vv.virtual_views_reference(sim.camera_poses(["zed_cam_left"]), small, None, BOX, FAR, [4], (2, 1024), 4), "one view of 2 x 1024, radius 4")
    both_equal_the_reference(sim, dev, CAMS2, H, W, depth, None, BOX, FAR, views, size, radius, "after the refusals")


def test_more_envs_than_a_chunk():
    """1027 envs go through the kernels as a chunk of 1024 and one of 3: depth, colour, out and index of the second chunk start at their own
    offsets.  One camera, 5 x 6, another depth image per env, two views at (4, 3)."""
    from av_aloha_amd.sim import BatchedSim
    from test_oracle_physics import OBJ
    n, H, W = 1027, 5, 6
    s = BatchedSim("slot_insertion", 3, n)
    try:
        s.reset(np.repeat(OBJ[None], n, 0))
        rng = np.random.default_rng(55)
        depth = rng.uniform(0.3, 1.5, (n, 1, H, W)).astype(np.float32)
        rgb = rng.integers(0, 256, (n, 1, H, W, 3), dtype=np.uint8)
        poses = s.camera_poses(["wrist_cam_right"])
        out, index = s.virtual_views(["wrist_cam_right"], H, W, BOX, ["+z", "-x"], (4, 3), radius=1, depth=depth, rgb=rgb)
        want = vv.virtual_views_reference(poses, depth, rgb, BOX, FAR, [4, 1], (4, 3), 1)
        assert out.shape == (n, 2, 4, 3, 8) and index.shape == (n, 2, 4, 3)
        assert out.view(np.int32).tobytes() == want[0].view(np.int32).tobytes() and index.tobytes() == want[1].tobytes()
        assert (want[1][1024:] >= 0).sum() > 30 and not np.array_equal(want[0][1024], want[0][0]) and not np.array_equal(want[1][1026], want[1][2])
    finally:
        s.close()


# ---- against avsim_voxel_grid and the renderers: no specification below this line -------------------------------------------------------------

def test_views_and_voxel_grid_agree(sim):
    """The pixel formula is the cell formula: seen from above at size (gy, gx) with radius 0, a pixel is hit exactly when some cell of its
    column of the grid is occupied; likewise from the lo-y face at size (gz, gx) against the maximum over y."""
    H, W, (gx, gy, gz) = 24, 32, (6, 5, 4)
    depth = noise_depth(56, 2, H, W)
    grid = sim.voxel_grid(CAMS2, H, W, BOX, (gx, gy, gz), depth=depth)
    top, _ = sim.virtual_views(CAMS2, H, W, BOX, ["+z"], (gy, gx), radius=0, depth=depth)
    side, _ = sim.virtual_views(CAMS2, H, W, BOX, ["-y"], (gz, gx), radius=0, depth=depth)
    assert grid[..., 7].sum() > 30
    for n in range(N):
        for i in range(gx):
            for j in range(gy):
                assert top[n, 0, gy - 1 - j, i, 7] == grid[n, i, j, :, 7].max(), (n, i, j)
            for k in range(gz):
                assert side[n, 0, gz - 1 - k, i, 7] == grid[n, i, :, k, 7].max(), (n, i, k)


def test_rendered_images(sim):
    """The depth and colour the renderers draw of the three arm configurations: wherever a pixel is hit its colour is the source pixel's and
    its point the deprojection's at `index`, and the view from above sees the scene."""
    H, W = 24, 32
    cams = ["zed_cam_left", "wrist_cam_right", "overhead_cam"]
    depth, rgb = sim.render_depth(cams, H, W), sim.render_rgb(cams, H, W, visual=False)
    poses = sim.camera_poses(cams)
    bounds = (-1.0, -1.0, -0.05, 1.0, 1.0, 1.5)
    out, index = sim.virtual_views(cams, H, W, bounds, ["+z", "+x", "-x", "+y", "-y"], (20, 20), radius=1, depth=depth, rgb=rgb)
    assert out.shape == (N, 5, 20, 20, 8) and index.shape == (N, 5, 20, 20)
    for n in range(N):
        hit = index[n] >= 0
        assert hit[0].sum() > 20, f"env {n}: the view from above has {int(hit[0].sum())} hits"
        slot = index[n][hit]
        colour = rgb[n].reshape(-1, 3)[slot].astype(np.float32) * np.float32(1.0 / 255.0)
        assert np.array_equal(out[n][hit][:, :3], colour)
        world = pc.deproject(poses[n], depth[n]).reshape(-1, 3)[slot]
        assert np.array_equal(out[n][hit][:, 4:7].view(np.int32), world.view(np.int32))
        assert (out[n][hit][:, 7] == 1).all() and not out[n][~hit].any()
    assert rgb.max() > 0 and out[..., :3].max() > 0


# ---- the layers above -------------------------------------------------------------------------------------------------------------------

SLOT = "gym_guided_vision/SlotInsertion-3Arms-v0"
VVARG = {"cameras": ["zed_cam_left", "wrist_cam_left"], "height": 24, "width": 32, "bounds": (-1.0, -1.0, -0.05, 1.0, 1.0, 1.5), "views": ["+z", "+x", "-y"], "size": (10, 12),
         "radius": 1, "colour": True}


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
    assert plain._vv is None and not any("virtual" in k for k in keys0 | info0) and "avsim_virtual_views" not in calls0 and not any("render" in c for c in calls0)
    plain.close()
    for fmt, key in (("lerobot", "observation.virtual_views"), ("gym", "virtual_views")):
        env = make_vec(SLOT, 4, 3, cameras=[], seed=2, obs_format=fmt, views=VVARG)
        calls = one_reset_and_step(env)
        assert calls.count("avsim_virtual_views") == 2 and [c for c in calls if c not in ("avsim_render_depth", "avsim_render_rgb", "avsim_virtual_views")] == calls0
        obs, info = env.reset()
        if fmt == "lerobot":
            assert set(obs) == keys0 | {key} and set(info) == info0 | {"virtual_views_index"}
        x, ix = obs[key], info["virtual_views_index"]
        assert x.dtype == T.float32 and tuple(x.shape) == (4, 3, 8, 10, 12) and x.device == env.device and x.stride() == (2880, 960, 1, 96, 8)
        assert ix.dtype == T.int32 and tuple(ix.shape) == (4, 3, 10, 12) and ix.device == env.device and ix.is_contiguous()
        a = env._ap.float().clone()
        a[:, 0] += 0.2
        a[:, 14] += 0.2
        last = None
        for t in range(1, 5):
            obs, r, te, tr, info = env.step(a)
            want, windex = env.virtual_views(VVARG["cameras"], 24, 32, VVARG["bounds"], VVARG["views"], VVARG["size"], radius=1, colour=True, channels_first=True)
            assert tuple(want.shape) == (4, 3, 8, 10, 12) and want.stride() == obs[key].stride() and T.equal(obs[key], want), (fmt, t)
            assert T.equal(info["virtual_views_index"], windex) and ((info["virtual_views_index"] >= 0) == (obs[key][:, :, 7] == 1)).all()
            assert (obs[key][:, 0, 7].sum((1, 2)) > 3).all() and obs[key][:, :, :3].max() > 0
            if t == 3:
                assert tr.all()
                last = obs[key].clone()
            if t == 4:          # NEXT_STEP autoreset: the new episode's first views, not the old episode's last
                assert (info["elapsed_steps"] == 0).all() and not T.equal(obs[key], last)
        env.close()
    both = make_vec(SLOT, 2, 3, cameras=[], views=VVARG, voxels={**{k: VVARG[k] for k in ("cameras", "height", "width", "bounds")}, "grid": 4},
                    pointcloud={**{k: VVARG[k] for k in ("cameras", "height", "width", "bounds")}, "points": 16})
    obs, info = both.reset()
    assert {"observation.virtual_views", "observation.voxels", "observation.pointcloud"} <= set(obs) and {"virtual_views_index", "pointcloud_index"} <= set(info)
    both.close()
    with pytest.raises(ValueError):
        make_vec(SLOT, 2, 3, cameras=[], views=VVARG, options={"render_cam_major": 1})
    with pytest.raises(ValueError):
        make_vec(SLOT, 2, 3, cameras=["zed_cam_left"], views=VVARG)
    with pytest.raises(ValueError):          # checked before there is a handle to give back
        make_vec(SLOT, 2, 3, cameras=[], views={**VVARG, "radius": 5})
