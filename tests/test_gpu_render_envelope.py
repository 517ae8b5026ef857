"""The three image kernels -- k_render_depth<false> (depth), k_render_depth<true> (proxy colour), k_vis_render (visual meshes) -- pixel by
pixel against sub-pixel envelopes of the oracle's f64 ray casters (tests/render_envelope.py; the rule is shown sound and sharp on the CPU
in tests/test_render_envelope_host.py): a device pixel must lie between the smallest and the largest of the oracle's nine rays within 0.2
pixel of its centre.  Interior pixels (depth spread of the nine rays <= 1 cm): none may fail.  Edge pixels: one per image, one per 10 000
compared pixels of a test function.

The states are kinematic (set_qpos on both sides: device and oracle hold the same pose) and sit in the envs of ONE batch, so that per-env
record indexing is exercised: S0 reset pose, S1 six wiggle steps, S2 / S3 the stick / the slot through the near plane of a wrist camera,
S4 the ZED cameras grazing the table with the frame's bars diagonal, S5 the stick cut by two image corners of overhead_cam and the camera
inside the slot; hook_package (cylinder) and tube_transfer (sphere) at the reset pose and with the object through a near plane."""
import numpy as np
import pytest

import render_envelope as RE
from orc_env import OrcEnv
from test_oracle_physics import model_dict

pytestmark = pytest.mark.gpu

SLOT_STATES = ["S0", "S1", "S2", "S3", "S4", "S5"]
OTHER = [("hook_package", "R0"), ("hook_package", "R2"), ("tube_transfer", "R0"), ("tube_transfer", "R2")]


class World:
    """One task: the oracle, the states, one device batch with a state per env, and what both sides rendered so far."""

    def __init__(self, task):
        from av_aloha_amd.sim import BatchedSim
        self.task, self.md, self.e = task, model_dict(task), OrcEnv(task, 3)
        self.S = RE.slot_states(self.e) if task == "slot_insertion" else RE.other_task_states(task, self.e)
        self.names = list(self.S)
        self.sim = self.batch(BatchedSim, True, 1e-12)
        self.sim32 = None
        self.cache = {}

    def batch(self, BatchedSim, f64, tol):
        sim = BatchedSim(self.task, 3, len(self.names), f64=f64)
        a0 = int(self.md["objects_qposadr"][0])
        sim.reset(np.repeat(self.md["qpos_home"][a0:][None], len(self.names), 0))
        sim.set_qpos(np.stack([self.S[n] for n in self.names]))
        assert np.abs(sim.get_state()[0] - np.stack([self.S[n] for n in self.names])).max() < tol
        return sim

    def device_f32(self, cams, H, W):
        """Depth images of the same states from a handle in the product mode (f32 state and poses; the other tests use the f64 handle)."""
        if self.sim32 is None:
            from av_aloha_amd.sim import BatchedSim
            self.sim32 = self.batch(BatchedSim, False, 1e-6)
        return self.sim32.render_depth(cams, H, W)

    def device(self, kind, cams, H, W, smooth=None):
        """The batch's images [N, len(cams), H, W(, 3)]: one render call per (kind, cameras, size), whichever state asks first."""
        key = ("dev", kind, tuple(cams), H, W, smooth)
        if key not in self.cache:
            if kind == "depth":
                self.cache[key] = self.sim.render_depth(cams, H, W)
            elif kind == "proxy":
                self.cache[key] = self.sim.render_rgb(cams, H, W, visual=False)
            else:
                self.sim.set_option("render_smooth", 1 if smooth else 0)
                self.cache[key] = self.sim.render_rgb(cams, H, W)
                assert self.sim.visual_info()["overflow"] == 0
        return self.cache[key]

    def oracle_at(self, state):
        if self.cache.get("at") != state:
            self.e.set_qpos(self.S[state])
            self.cache["at"] = state

    def proxy(self, state, cam, H, W):
        """(colour envelope, depth envelope): one high-resolution pass of the oracle serves the depth and the colour tests."""
        key = ("proxy", state, cam, H, W)
        if key not in self.cache:
            self.oracle_at(state)
            self.cache[key] = RE.proxy_envelope(self.e, cam, H, W)
        return self.cache[key]

    def depth_rows(self, state, cam, H, W, rows):
        self.oracle_at(state)
        return RE.depth_envelope(self.e, cam, H, W, rows=rows)

    def close(self):
        self.sim.close()
        if self.sim32 is not None:
            self.sim32.close()
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


def label(w, state, cam, H, W, what):
    return f"{w.task} {state} (env {w.names.index(state)}) {cam} {H}x{W} {what}"


@pytest.mark.parametrize("task,state", [("slot_insertion", s) for s in SLOT_STATES] + OTHER)
def test_depth_every_state_all_cameras(worlds, task, state):
    H, W = 60, 80
    w = worlds(task)
    img = w.device("depth", RE.CAMS, H, W)
    assert img.shape == (len(w.names), 6, H, W) and img.dtype == np.float32
    t = RE.Tally()
    for ci, cam in enumerate(RE.CAMS):
        t.add(img[w.names.index(state), ci], w.proxy(state, cam, H, W)[1], RE.TOL_DEPTH, label(w, state, cam, H, W, "depth"))
    print(f"{task} {state} depth 60x80: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


@pytest.mark.parametrize("task", ["slot_insertion", "hook_package", "tube_transfer"])
def test_depth_every_state_all_cameras_f32_handle(worlds, task):
    """The same images from a handle in the product mode: its f32 poses are off the oracle's by the order of 1e-6, the noise the envelopes are
    shown to absorb (tests/test_render_envelope_host.py)."""
    H, W = 60, 80
    w = worlds(task)
    img = w.device_f32(RE.CAMS, H, W)
    t = RE.Tally()
    for state in w.names:
        for ci, cam in enumerate(RE.CAMS):
            t.add(img[w.names.index(state), ci], w.proxy(state, cam, H, W)[1], RE.TOL_DEPTH, label(w, state, cam, H, W, "depth, f32 handle"))
    print(f"{task} depth 60x80, f32 handle: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


# tile = 32 x 16 pixels, bin = at most 10 x 2 tiles in equally wide columns, bin masks of 128 bits
SMALL = [(1, 1), (16, 32), (17, 33)]            # the whole scene in one tile of one bin (longest list, the arena cannot hold every polyhedron); ragged both ways, width not a multiple of 4
WIDE = (48, 352)                                # 11 tile columns -> bin columns of 6 and 5; 3 tile rows -> a ragged second bin row
TALL = [(2048, 352), (2080, 352)]               # 64 x 2 = 128 bins: the last mask bit; 65 x 2 = 130 bins: the all-ones fallback
SHAPE_CAMS = ["wrist_cam_right", "zed_cam_left", "overhead_cam"]


@pytest.mark.parametrize("state", ["S0", "S2", "S4"])
def test_depth_small_shapes(worlds, state):
    w = worlds("slot_insertion")
    t = RE.Tally()
    for H, W in SMALL:
        img = w.device("depth", RE.CAMS, H, W)
        for ci, cam in enumerate(RE.CAMS):
            t.add(img[w.names.index(state), ci], w.proxy(state, cam, H, W)[1], RE.TOL_DEPTH, label(w, state, cam, H, W, "depth"))
    print(f"{state} depth small shapes: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


@pytest.mark.parametrize("state", ["S0", "S2", "S4"])
def test_depth_two_bin_columns(worlds, state):
    """Every pixel of 48 x 352, the state's own camera and one other."""
    H, W = WIDE
    w = worlds("slot_insertion")
    cams = ["zed_cam_left", "overhead_cam" if state == "S0" else "wrist_cam_right"]
    img = w.device("depth", SHAPE_CAMS, H, W)
    t = RE.Tally()
    for cam in cams:
        w.oracle_at(state)
        t.add(img[w.names.index(state), SHAPE_CAMS.index(cam)], RE.depth_envelope(w.e, cam, H, W), RE.TOL_DEPTH, label(w, state, cam, H, W, "depth"))
    print(f"{state} depth 48x352: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


@pytest.mark.parametrize("hw", TALL)
@pytest.mark.parametrize("state", ["S0", "S2", "S4"])
def test_depth_bin_masks_to_their_last_bit_and_beyond(worlds, state, hw):
    """Twelve strided rows, the first row and the last one (last tile row, last bin row) of three cameras."""
    H, W = hw
    w = worlds("slot_insertion")
    img = w.device("depth", SHAPE_CAMS, H, W)
    assert np.isfinite(img).all()
    step = H // 12
    t = RE.Tally()
    for ci, cam in enumerate(SHAPE_CAMS):
        for rows in ((7, step, 12), (0, 1, 1), (H - 1, 1, 1)):
            r0, st, n = rows
            t.add(img[w.names.index(state), ci, r0::st][:n], w.depth_rows(state, cam, H, W, rows), RE.TOL_DEPTH, label(w, state, cam, H, W, "depth"), rows=rows)
    print(f"{state} depth {H}x{W}: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


@pytest.mark.parametrize("task,state", [("slot_insertion", "S0"), ("slot_insertion", "S2"), ("slot_insertion", "S5")] + OTHER)
def test_proxy_colour(worlds, task, state):
    """render_rgb(visual=False) at 60 x 80, 17 x 33 (bytewise stores) and 16 x 32, all six cameras: +-1 level about the envelope."""
    w = worlds(task)
    t = RE.Tally()
    for H, W in [(60, 80), (17, 33), (16, 32)]:
        img = w.device("proxy", RE.CAMS, H, W)
        assert img.shape == (len(w.names), 6, H, W, 3) and img.dtype == np.uint8
        for ci, cam in enumerate(RE.CAMS):
            t.add(img[w.names.index(state), ci], w.proxy(state, cam, H, W)[0], RE.TOL_PROXY, label(w, state, cam, H, W, "proxy colour"))
    print(f"{task} {state} proxy colour: {t.interior} interior, {t.edge} edge pixels outside the envelope of {t.compared}")
    t.done()


@pytest.fixture(scope="module")
def scene():
    return RE.scene_of("slot_insertion", 3)


@pytest.mark.parametrize("smooth", [True, False])
@pytest.mark.parametrize("cam", RE.VIS_CAMS)
@pytest.mark.parametrize("state", ["S0", "S2"])
def test_visual_meshes(worlds, scene, state, cam, smooth):
    """render_rgb of the visual meshes at 40 x 56, K = 3, +-2 levels about the envelope.  The device rasterises with an f32 test on 1 / depth,
    the oracle casts one f64 ray per pixel: where two surfaces nearly coincide the two may differ away from any edge, and so may the
    oracle from itself under pose noise.  Interior pixels outside the envelope: at most three times the count of the oracle's own image
    under 1e-6 noise (render_envelope.visual_reference, seed 0) plus 2 -- below the stick's 11 pixels in the overhead view; the edge rule as
    everywhere.

    Measured (interior / edge pixels outside the envelope, of 2240 per image; S0 and S2, smooth and flat alike):
        overhead_cam      oracle under noise 0 / 0    device 0 / 0
        wrist_cam_right   oracle under noise 0 / 0    device 0 / 0
        zed_cam_left      oracle under noise 0 / 0    device 1 / 0   (pixel (16, 50): device grey 38, envelope 28 .. 34)
    That pixel is not a hole: the oracle at K = 9 shows a sliver triangle of the right gripper base's mesh with grey 38, one ray (0.11 pixel)
    to the right of the pixel's centre and in no other ray of the block -- narrower than the K = 3 rays are apart, at the same depth (0.2860 m
    against 0.2859 m), so the pixel counts as interior."""
    H, W = RE.VIS_HW
    w = worlds("slot_insertion")
    img = w.device("visual", RE.VIS_CAMS, H, W, smooth=smooth)
    assert img.shape == (len(w.names), 3, H, W, 3)
    env, _, (ri, re_) = RE.visual_reference(w.md, w.e, scene, w.S[state], cam, smooth)
    w.cache["at"] = state
    t = RE.Tally(interior_allowed=3 * ri + 2)
    ni, ne = t.add(img[w.names.index(state), RE.VIS_CAMS.index(cam)], env, RE.TOL_VISUAL, label(w, state, cam, H, W, "visual smooth" if smooth else "visual flat"))
    print(f"{state} {cam} {'smooth' if smooth else 'flat'}: oracle under noise {ri} interior / {re_} edge, device {ni} interior / {ne} edge pixels outside the envelope")
    t.done()
