"""avsim_render_labels on the device (k_render_depth's labels mode; av_aloha_amd/segment.py is the specification): the label image against
the f64 reference cast through the sub-pixel rule of tests/segment_util.py, the depth image against avsim_render_depth bit for bit, drop,
optional outputs, tables, chunked passes, both I/O modes with guard words, the refusals, and the vector env's options.

Every batch has N = 3 envs in three different states.  Sizes (segment_util.SIZES): 30 x 40 -- one partly filled tile, a row's four labels
in one 32-bit store; 33 x 42 -- W % 4 != 0, single bytes, three tile rows over two bin rows; 24 x 332 -- 11 tiles across, two bin columns.
States: zed_cam_left on S0 / S1, wrist_cam_left on S3 (a polyhedron through the near plane: the general path), overhead_cam on S5 (the
camera inside a geom), wrist_cam_right on R2 of hook_package (cylinder) and tube_transfer (sphere)."""
import numpy as np
import pytest

import render_envelope as RE
import segment_util as SU
from av_aloha_amd import _ffi, segment
from av_aloha_amd.sim import BatchedSim
from gpu_util import Guarded, device_handle_in_state, torch as T
from orc_env import OrcEnv
from test_oracle_physics import model_dict

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 0x5A
GUARD = 1024            # bytes before an output: a multiple of 16, as the call wants a depth image aligned with W % 4 == 0
FAR = np.float32(RE.FAR)
SLOT_CAMS = ["zed_cam_left", "wrist_cam_left", "overhead_cam"]
EINVAL = -1


class World:
    """One task: the oracle, the states, one f64 device batch of three envs (device and oracle hold the same poses)."""

    def __init__(self, task):
        self.task, self.md, self.e = task, model_dict(task), OrcEnv(task, 3)
        self.S = SU.states_of(task, self.e)
        self.sim = BatchedSim(task, 3, N, f64=True)
        a0 = int(self.md["objects_qposadr"][0])
        self.sim.reset(np.repeat(self.md["qpos_home"][a0:][None], N, 0))
        self.states = None
        self.cache = {}

    def use(self, states):
        if self.states != tuple(states):
            q = np.stack([self.S[s] for s in states])
            self.sim.set_qpos(q)
            assert np.abs(self.sim.get_state()[0] - q).max() < 1e-12
            self.states = tuple(states)

    def accepted(self, state, cam, H, W, table):
        key = (state, cam, H, W)
        if key not in self.cache:
            self.e.set_qpos(self.S[state])
            self.cache[key] = SU.nine_rays(self.md, self.e, cam, H, W)
        return SU.accepted(self.cache[key], table)

    def close(self):
        self.sim.close()
        self.e.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(task):
        if task not in made:
            made[task] = World(task)
        return made[task]
    yield get
    for w in made.values():
        w.close()


SLOT_STATES = ("S0", "S3", "S5")


@pytest.fixture
def slot(worlds):
    w = worlds("slot_insertion")
    w.use(SLOT_STATES)
    return w


@pytest.mark.parametrize("size", SU.SIZES)
@pytest.mark.parametrize("task,states,env,cam", SU.CASES)
def test_labels_against_the_reference_cast(worlds, task, states, env, cam, size):
    """The geom image (identity table) under the rule: a pixel with one accepted label carries it, one with several carries one of them
    (one per image and one per 10 000 compared aside).  The depth of the same call is avsim_render_depth's, bit for bit."""
    H, W = size
    w = worlds(task)
    w.use(states)
    lab, dep = w.sim.render_labels([cam], H, W, kind="geom")
    assert lab.dtype == np.uint8 and lab.shape == (N, 1, H, W) and dep.dtype == np.float32 and dep.shape == lab.shape
    assert np.array_equal(dep, w.sim.render_depth([cam], H, W))
    table, _ = segment.label_table(w.sim.manifest, w.md, "geom")
    acc = w.accepted(states[env], cam, H, W, table)
    share = SU.single_share(acc)
    print(f"{task} {states[env]} {cam} {H}x{W}: {100 * share:.1f} % of the pixels have one accepted label")
    assert share >= SU.MIN_SINGLE
    t = SU.LabelTally()
    print("(single, several) accepted labels missed:", t.add(lab[env, 0], acc, f"{task} {states[env]} (env {env}) {cam} {H}x{W}"))
    t.done()
    # nothing <=> the far plane; every label is a visible geom's
    assert np.array_equal(lab == 255, dep == FAR)
    seen = np.unique(lab[lab != 255])
    assert len(seen) > 1 and (np.asarray(w.md["geom_visible"]).reshape(-1)[seen] == 1).all()


@pytest.mark.parametrize("size", SU.SIZES)
def test_depth_drop_optional_outputs_and_tables(slot, size):
    """All three cameras in one call, per size: depth = avsim_render_depth bit for bit; with drop exactly the pixels of a dropped label hold
    30.0 and the others are unchanged; depth=None / labels=None give the other output unchanged; table NULL is the identity; the class
    image is the geom image through the class table."""
    H, W = size
    sim, L, h = slot.sim, slot.sim.h.L, slot.sim.h.h
    ids = np.array([sim.manifest["camera_names"].index(c) for c in SLOT_CAMS], dtype=np.int32)
    ref = sim.render_depth(SLOT_CAMS, H, W)
    geom, dep = sim.render_labels(SLOT_CAMS, H, W, kind="geom")
    assert np.array_equal(dep, ref)
    shape = (N, 3, H, W)
    cls, names = sim.label_table("class")
    robot = [names.index(c) for c in segment.ROBOT_CLASSES]
    lab, dropped = sim.render_labels(SLOT_CAMS, H, W, drop=segment.ROBOT_CLASSES)
    assert np.array_equal(lab, cls[np.minimum(geom, len(cls) - 1)]) and np.array_equal(lab == 0, geom == 255)
    gone = np.isin(lab, robot)
    assert 0.02 < gone.mean() < 0.9 and (dropped[gone] == FAR).all() and np.array_equal(dropped[~gone], ref[~gone])
    assert (ref[gone] < FAR).all()
    # drop by value through a table of the caller's, one output at a time
    flags = segment.drop_flags(robot)
    only_lab, only_dep = np.full(shape, SENTINEL, dtype=np.uint8), np.full(shape, np.nan, dtype=np.float32)
    assert L.avsim_render_labels(h, ids.ctypes.data, 3, H, W, cls.ctypes.data, None, None, only_lab.ctypes.data) == 0
    assert L.avsim_render_labels(h, ids.ctypes.data, 3, H, W, cls.ctypes.data, flags.ctypes.data, only_dep.ctypes.data, None) == 0
    assert np.array_equal(only_lab, lab) and np.array_equal(only_dep, dropped)
    # table NULL
    null_lab, null_dep = np.full(shape, SENTINEL, dtype=np.uint8), np.full(shape, np.nan, dtype=np.float32)
    assert L.avsim_render_labels(h, ids.ctypes.data, 3, H, W, None, None, null_dep.ctypes.data, null_lab.ctypes.data) == 0
    assert np.array_equal(null_lab, geom) and np.array_equal(null_dep, ref)
    # the body table, and both register forms of the kernel
    body, _ = sim.render_labels(SLOT_CAMS, H, W, kind="body", depth=False)
    assert np.array_equal(body[geom != 255], np.asarray(slot.md["geom_body"]).reshape(-1)[geom[geom != 255]]) and (body[geom == 255] == 255).all()
    sim.set_option("render_labels_form", 1)
    try:
        lab1, dropped1 = sim.render_labels(SLOT_CAMS, H, W, drop=segment.ROBOT_CLASSES)
    finally:
        sim.set_option("render_labels_form", 0)
    assert np.array_equal(lab1, lab) and np.array_equal(dropped1, dropped)


def test_chunked_passes(slot):
    """Option "render_chunk" 2 with N = 3: two passes, the second one's label offset in bytes and its depth offset in floats."""
    sim = slot.sim
    for H, W in SU.SIZES[:2]:
        want = sim.render_labels(SLOT_CAMS, H, W, drop=["left_arm", "slot"])
        sim.set_option("render_chunk", 2)
        try:
            got = sim.render_labels(SLOT_CAMS, H, W, drop=["left_arm", "slot"])
            only = sim.render_labels(SLOT_CAMS, H, W, depth=False)
        finally:
            sim.set_option("render_chunk", 4096)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(only[0], want[0]) and only[1] is None
        assert len({want[0][n].tobytes() for n in range(N)}) == N


class Dev:
    """A device-mode f64 handle of the slot model in the world's states, outputs in the middle of sentinel-filled tensors."""

    def __init__(self, qpos):
        md = model_dict()
        a0 = int(md["objects_qposadr"][0])
        self.h, self.d = device_handle_in_state("slot_insertion", N, np.repeat(md["qpos_home"][a0:][None], N, 0), qpos, _ffi.AVSIM_F64_PHYSICS)

    def labels(self, ids, H, W, table=None, drop=None, depth=True, labels=True, ncam=None, cam_ids=True, offset=0):
        """-> (rc, labels, depth, every byte around the two outputs is the sentinel, the outputs are all sentinels)."""
        npx = N * len(ids) * H * W
        b_lab = Guarded(self.d, npx, T.uint8, SENTINEL, GUARD, 1024)
        b_dep = Guarded(self.d, 4 * npx, T.uint8, SENTINEL, GUARD, 1024)
        rc = self.h.L.avsim_render_labels(self.h.h, ids.ctypes.data if cam_ids else None, len(ids) if ncam is None else ncam, H, W,
                                          None if table is None else table.ctypes.data, None if drop is None else drop.ctypes.data,
                                          b_dep.ptr(offset) if depth else None, b_lab.ptr(offset) if labels else None)
        T.cuda.synchronize()
        (body_l, intact_l, same_l), (body_d, intact_d, same_d) = b_lab.read(), b_dep.read()
        return rc, body_l.reshape(N, len(ids), H, W), body_d.view(np.float32).reshape(N, len(ids), H, W), intact_l and intact_d, same_l and same_d


@pytest.fixture(scope="module")
def dev(worlds):
    slot = worlds("slot_insertion")
    d = Dev(np.stack([slot.S[s] for s in SLOT_STATES]))
    yield d
    d.h.close()


@pytest.mark.parametrize("size", SU.SIZES)
def test_both_io_modes_agree_and_guards_are_intact(slot, dev, size):
    H, W = size
    sim = slot.sim
    ids = np.array([sim.manifest["camera_names"].index(c) for c in SLOT_CAMS], dtype=np.int32)
    cls, names = sim.label_table("class")
    flags = segment.drop_flags(["right_arm", "stick", "frame"], names)
    want_lab, want_dep = sim.render_labels(SLOT_CAMS, H, W, drop=["right_arm", "stick", "frame"])
    rc, lab, dep, guards, _ = dev.labels(ids, H, W, cls, flags)
    assert rc == 0 and guards and np.array_equal(lab, want_lab) and np.array_equal(dep, want_dep)
    rc, lab, dep, guards, _ = dev.labels(ids, H, W, cls, None, depth=False)
    assert rc == 0 and guards and np.array_equal(lab, want_lab) and (dep.view(np.uint8) == SENTINEL).all()
    rc, lab, dep, guards, _ = dev.labels(ids, H, W, cls, flags, labels=False)
    assert rc == 0 and guards and np.array_equal(dep, want_dep) and (lab == SENTINEL).all()


def test_refusals_leave_the_outputs_untouched(slot, dev):
    H, W = 30, 40
    ncam_model = len(slot.sim.manifest["camera_names"])
    ids = np.array([2, 0], dtype=np.int32)
    drop = np.zeros(256, dtype=np.uint8)
    cases = [("no cameras", dict(ncam=0)), ("17 cameras", dict(ncam=17)), ("camera id out of range", dict(ids=np.array([2, ncam_model], dtype=np.int32))),
             ("negative camera id", dict(ids=np.array([-1, 0], dtype=np.int32))), ("height 0", dict(H=0)), ("width 0", dict(W=0)), ("height 4097", dict(H=4097)),
             ("width 4097", dict(W=4097)), ("null cam_ids", dict(cam_ids=False)), ("both outputs null", dict(depth=False, labels=False)),
             ("drop without depth", dict(drop=drop, depth=False)), ("misaligned outputs", dict(offset=2))]
    for what, kw in cases:
        a = dict(ids=ids, H=H, W=W)
        a.update(kw)
        # (the buffers are sized for the good call: a refused size launches nothing, so nothing is written)
        npx = N * 2 * 30 * 40
        b_lab = Guarded(dev.d, npx, T.uint8, SENTINEL, GUARD, 1024)
        b_dep = Guarded(dev.d, 4 * npx, T.uint8, SENTINEL, GUARD, 1024)
        off = a.get("offset", 0)
        rc = dev.h.L.avsim_render_labels(dev.h.h, a["ids"].ctypes.data if a.get("cam_ids", True) else None, a.get("ncam", len(a["ids"])), a["H"], a["W"], None,
                                         a["drop"].ctypes.data if "drop" in a else None, b_dep.ptr(off) if a.get("depth", True) else None,
                                         b_lab.ptr(off) if a.get("labels", True) else None)
        T.cuda.synchronize()
        assert rc == EINVAL, what
        assert all(b_lab.read()[1:]) and all(b_dep.read()[1:]), what
        assert dev.h.L.avsim_last_error(dev.h.h), what
    # the fronts refuse the same before they allocate, as a ValueError; a good call still works afterwards
    for kw in (dict(cameras=[]), dict(cameras=[ncam_model]), dict(height=0), dict(width=4097), dict(drop=["left_arm"], depth=False), dict(kind=np.zeros(3, dtype=np.uint8)),
               dict(drop=["arm"])):
        a = dict(cameras=["zed_cam_left"], height=H, width=W)
        a.update(kw)
        with pytest.raises(ValueError):
            slot.sim.render_labels(**a)
    rc, lab, dep, guards, untouched = dev.labels(ids, H, W)
    assert rc == 0 and guards and not untouched and np.array_equal(dep, slot.sim.render_depth(["zed_cam_left", "wrist_cam_left"], H, W))


def test_facade_render_segmentation():
    from av_aloha_amd.env import SlotInsertionEnv
    env = SlotInsertionEnv(num_arms=3, cameras=[])
    env.reset(seed=0)
    seg = env.render_segmentation(["zed_cam_left", "overhead_cam"], 30, 40)
    dep = env.render_depth(["zed_cam_left", "overhead_cam"], 30, 40)
    names = env.sim.label_table("class")[1]
    for cam in seg:
        assert seg[cam].dtype == np.uint8 and seg[cam].shape == (30, 40) and np.array_equal(seg[cam] == 0, dep[cam] == FAR)
    assert {names[l] for l in np.unique(seg["overhead_cam"])} >= {"table", "left_arm", "right_arm", "slot", "stick"}
    env.close()


SLOT = "gym_guided_vision/SlotInsertion-3Arms-v0"
PCARG = {"cameras": ["zed_cam_left", "overhead_cam"], "height": 30, "width": 40, "bounds": (-1.0, -1.0, -0.05, 1.0, 1.0, 1.5), "points": 64}
SEGARG = {"cameras": ["zed_cam_left", "wrist_cam_left"], "height": 33, "width": 42, "kind": "class"}


def test_vector_env_options():
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

    # no new option: the keys and calls of the parent
    plain = make_vec(SLOT, N, 50, cameras=[], seed=2, pointcloud=PCARG)
    obs0, info0 = plain.reset()
    keys0, ikeys0 = set(obs0), set(info0)
    calls0 = one_reset_and_step(plain)
    assert keys0 == {"observation.state", "observation.pointcloud"} and ikeys0 == {"episode_id", "elapsed_steps", "is_success", "pointcloud_count", "pointcloud_index"}
    assert "avsim_render_labels" not in calls0 and calls0.count("avsim_render_depth") == 2 and plain._seg is None and not hasattr(plain, "segmentation_classes")
    assert plain._pc["labels"] is None and plain._pc["table"] is None
    plain.close()

    robot = list(segment.ROBOT_CLASSES)
    for fmt in ("lerobot", "gym"):
        env = make_vec(SLOT, N, 50, cameras=[], seed=2, obs_format=fmt, pointcloud={**PCARG, "drop": robot, "labels": True}, segmentation=SEGARG)
        names = env.segmentation_classes
        assert names[:8] == segment.FIXED_CLASSES and names[8:] == ["slot", "stick"]
        calls = one_reset_and_step(env)
        assert calls.count("avsim_render_labels") == 4 and "avsim_render_depth" not in calls and [c for c in calls if c != "avsim_render_labels"] == [c for c in calls0 if c != "avsim_render_depth"]
        obs, info = env.reset()
        a = env._ap.float().clone()
        a[:, 0] += 0.2
        a[:, 14] += 0.2
        for t in range(2):
            if fmt == "lerobot":
                assert set(obs) == keys0 | {"observation.segmentation"} and set(info) - {"diverged"} == ikeys0 | {"pointcloud_label"}
                seg = obs["observation.segmentation"]
            else:
                assert set(obs["segmentation"]) == set(SEGARG["cameras"])
                seg = T.stack([obs["segmentation"][c] for c in SEGARG["cameras"]], 1)
                assert all(tuple(v.shape) == (N, 33, 42) and v.dtype == T.uint8 for v in obs["segmentation"].values())
            want, _ = env.render_labels(SEGARG["cameras"], 33, 42, kind="class", depth=False)
            assert seg.dtype == T.uint8 and tuple(seg.shape) == (N, 2, 33, 42) and T.equal(seg, want) and len(T.unique(seg)) >= 5
            # the cloud of the masked depth; its labels hold no dropped class
            lab, masked = env.render_labels(PCARG["cameras"], 30, 40, drop=robot)
            plain_depth = T.empty_like(masked)
            ids = np.array([env.manifest["camera_names"].index(c) for c in PCARG["cameras"]], dtype=np.int32)
            env.h.check(env.L.avsim_render_depth(env.h.h, ids.ctypes.data, 2, 30, 40, plain_depth.data_ptr()))
            gone = T.isin(lab, T.tensor([names.index(c) for c in robot], dtype=T.uint8, device=env.device))
            assert gone.any() and (masked[gone] == 30.0).all() and T.equal(masked[~gone], plain_depth[~gone])
            xyz, index, count = env.point_cloud(PCARG["cameras"], 30, 40, PCARG["bounds"], 64, depth=masked)
            key = "observation.pointcloud" if fmt == "lerobot" else "pointcloud"
            assert T.equal(obs[key], xyz) and T.equal(info["pointcloud_index"], index) and T.equal(info["pointcloud_count"], count)
            pl = info["pointcloud_label"]
            assert pl.dtype == T.uint8 and tuple(pl.shape) == (N, 64) and (count[:, 1] > 8).all()
            assert T.equal(pl, T.where(index >= 0, lab.view(N, -1).gather(1, index.clamp(min=0).long()), T.full_like(pl, 255)))
            assert not T.isin(pl, T.tensor([names.index(c) for c in robot], dtype=T.uint8, device=env.device)).any()
            # without the drop the same cloud sits partly on the robot
            xyz2, index2, _ = env.point_cloud(PCARG["cameras"], 30, 40, PCARG["bounds"], 64, depth=plain_depth)
            assert gone.view(N, -1).gather(1, index2.clamp(min=0).long()).any()
            obs, r, te, tr, info = env.step(a)
        env.close()

    # voxels and views take the drop list too: the grid / the views of the masked depth
    box = {k: PCARG[k] for k in ("cameras", "height", "width", "bounds")}
    env = make_vec(SLOT, N, 50, cameras=[], seed=2, voxels={**box, "grid": 6, "drop": robot}, views={**box, "views": ["+z", "-y"], "size": (10, 12), "colour": False, "drop": robot})
    obs, info = env.reset()
    _, masked = env.render_labels(PCARG["cameras"], 30, 40, drop=robot)
    assert T.equal(obs["observation.voxels"], env.voxel_grid(PCARG["cameras"], 30, 40, PCARG["bounds"], 6, depth=masked, channels_first=True))
    want, windex = env.virtual_views(PCARG["cameras"], 30, 40, PCARG["bounds"], ["+z", "-y"], (10, 12), depth=masked, channels_first=True)
    assert T.equal(obs["observation.virtual_views"], want) and T.equal(info["virtual_views_index"], windex)
    unmasked = env.voxel_grid(PCARG["cameras"], 30, 40, PCARG["bounds"], 6, channels_first=True)
    assert obs["observation.voxels"][:, 6].sum() < unmasked[:, 6].sum()
    env.close()
    with pytest.raises(ValueError):
        make_vec(SLOT, N, 50, cameras=[], pointcloud={**PCARG, "drop": ["robot"]})
    with pytest.raises(ValueError):
        make_vec(SLOT, N, 50, cameras=[], segmentation={**SEGARG, "height": 0})
