"""The image every facade hands out -- visual meshes with render_shadows 1, render_samples 4, render_smooth 1: k_vis_render<2, true, true>
behind k_vis_shadow -- pixel by pixel against the envelope of the oracle's f64 model of the depth-map shadow (DESIGN.md "The renderer's
shadow contract", oracle/orc_vis.c orc_vis_render_model, tests/render_envelope.py production_envelope; shown sound and sharp on the CPU in
tests/test_render_envelope_host.py), with a state per env, and at the batch sizes where k_vis_shadow's launch shape changes and
k_vis_render's workgroups reuse their scratch slots.

The states H0 .. H4 (render_envelope.shadow_states) are kinematic: set_qpos on both sides.  Images are 40 x 56 (VIS_HW) of VIS_CAMS.

Rule per image (render_envelope.Tally): +-2 levels about the envelope (TOL_VISUAL); interior pixels outside: at most three times the model's
own count under 1e-6 pose noise (production_reference, seed 0) plus 2; edge pixels outside: one per image and one per 10 000 compared pixels
of a test function.

Wall time on the CPU of the oracle's part, measured: one model render of 40 x 56 with four samples 13 ms, a 512-texel map 11 ms, an envelope
(nine renders) with its noise image 0.17 s; the thirty envelopes of the per-env tests 5 s in all; a 2048-texel map 0.2 s."""
import numpy as np
import pytest

import render_envelope as RE
from orc_env import OrcEnv
from test_oracle_physics import model_dict

pytestmark = pytest.mark.gpu

STATES = RE.SHADOW_STATES
H, W = RE.VIS_HW
BATCHES = [32, 64, 128, 256, 300]          # k_vis_shadow over 8, 4, 2, 1 and 1 bands of rows; 3 N views: from N = 128 on more than any GPU has CUs


class World:
    def __init__(self):
        self.md, self.e, self.scene = model_dict(), OrcEnv("slot_insertion", 3), RE.scene_of("slot_insertion", 3)
        self.S, self.facts = RE.shadow_states(self.e, self.scene)
        self.small = self.batch(len(STATES))
        self.cache = {}

    def batch(self, N):
        """N envs, env j in state j mod 5, f64 state (device and oracle hold the same pose), the facades' render options."""
        from av_aloha_amd.sim import BatchedSim
        sim = BatchedSim("slot_insertion", 3, N, f64=True)
        a0 = int(self.md["objects_qposadr"][0])
        sim.reset(np.repeat(self.md["qpos_home"][a0:][None], N, 0))
        q = np.stack([self.S[STATES[j % len(STATES)]] for j in range(N)])
        sim.set_qpos(q)
        assert np.abs(sim.get_state()[0] - q).max() < 1e-12
        sim.set_option("render_shadows", 1)
        sim.set_option("render_samples", 4)
        return sim

    def render(self, sim, smooth, **kw):
        sim.set_option("render_smooth", 1 if smooth else 0)
        img = sim.render_rgb(RE.VIS_CAMS, H, W, **kw)
        assert sim.visual_info()["overflow"] == 0
        return img

    def small_images(self, smooth):
        """[5, 3, H, W, 3]: the five states, one per env."""
        if ("dev", smooth) not in self.cache:
            self.cache["dev", smooth] = self.render(self.small, smooth)
        return self.cache["dev", smooth]

    def reference(self, state, cam, smooth, shn=RE.SHADOW_SIZE):
        key = ("ref", state, cam, smooth, shn)
        if key not in self.cache:
            self.cache[key] = RE.production_reference(self.md, self.e, self.scene, self.S[state], cam, smooth, shn)
        return self.cache[key]

    def close(self):
        self.small.close()
        self.e.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def fails(img, env, allowed):
    bi, be = RE.violations(img, env, RE.TOL_VISUAL)
    return int(bi.sum()) > allowed or int(be.sum()) > 1


@pytest.mark.parametrize("smooth", [True, False])
def test_every_env_against_the_envelope_of_its_own_state(world, smooth):
    """One batch, H0 .. H4 in envs 0 .. 4, shadows 1, samples 4: every env's image of every camera inside the envelope of ITS state -- and, in
    some camera, outside the envelope of at least one other state, so that no exchange of envs (poses, shadow maps, images) can pass.

    Measured (interior / edge pixels outside the envelope, of 2240 per image; the test prints every image's): the model under noise 0 / 0
    in 27 of the 30 images and 0 / 1 in three (wrist_cam_right: H1 smooth, H0 and H2 flat); the device 0 / 0 in 27 and 0 / 1 in three:
    H3 overhead_cam (20, 33), smooth and flat, where four triangles of the right gripper's silhouette meet over the table (blue 31 against
    38 .. 59; the image without shadows differs there likewise: coverage, not shadow), and H1 wrist_cam_right (14, 30) smooth, a sliver of
    the left gripper against the sky, 3 levels above.  In all 0 interior and 2 (smooth) / 1 (flat) edge pixels of 33 600; allowed 3.
    Before the model drew a triangle cut by the near plane as the device does (fragments) the table's seam under wrist_cam_right
    added three pixels 4 levels outside."""
    img = world.small_images(smooth)
    assert img.shape == (len(STATES), len(RE.VIS_CAMS), H, W, 3) and img.dtype == np.uint8
    mode = "smooth" if smooth else "flat"
    t = RE.Tally()
    for i, state in enumerate(STATES):
        for ci, cam in enumerate(RE.VIS_CAMS):
            env, _, (ri, re_) = world.reference(state, cam, smooth)
            t.interior_allowed = 3 * ri + 2
            ni, ne = t.add(img[i, ci], env, RE.TOL_VISUAL, f"{state} (env {i}) {cam} {H}x{W} shadows 1 samples 4 {mode}")
            print(f"{state} {cam} {mode}: model under noise {ri} interior / {re_} edge, device {ni} interior / {ne} edge pixels outside the envelope")
    t.done()
    for i, state in enumerate(STATES):
        told_apart = [other for other in STATES if other != state and
                      any(fails(img[i, ci], world.reference(other, cam, smooth)[0], 3 * world.reference(other, cam, smooth)[2][0] + 2) for ci, cam in enumerate(RE.VIS_CAMS))]
        print(f"{state} {mode}: its image fails the envelopes of {told_apart}")
        assert told_apart, f"the image of env {i} ({state}) passes every other state's envelope"


@pytest.mark.parametrize("shn", [1024, 2048])
def test_finer_shadow_maps(world, shn):
    """render_shadow_size 1024 and 2048 (the texel scale, the bias and the map's size change): H1 in overhead_cam against the model with a map
    of as many texels."""
    state, cam, smooth = "H1", "overhead_cam", True
    sim = world.small
    try:
        sim.set_option("render_shadow_size", shn)
        img = world.render(sim, smooth)
    finally:
        sim.set_option("render_shadow_size", RE.SHADOW_SIZE)
    env, _, (ri, re_) = world.reference(state, cam, smooth, shn)
    t = RE.Tally(interior_allowed=3 * ri + 2)
    ni, ne = t.add(img[STATES.index(state), RE.VIS_CAMS.index(cam)], env, RE.TOL_VISUAL, f"{state} {cam} shadow map {shn}")
    print(f"{state} {cam} shadow map {shn}: model under noise {ri} interior / {re_} edge, device {ni} interior / {ne} edge pixels outside the envelope")
    assert not np.array_equal(img, world.small_images(smooth))
    t.done()


def assert_replicas_equal(img, small, what):
    """img [N, 3, H, W, 3] of a batch whose env j holds state j mod 5 against the five-env batch's images, byte for byte."""
    unequal = [j for j in range(img.shape[0]) if not np.array_equal(img[j], small[j % len(STATES)])]
    print(f"{what}: {img.shape[0] - len(unequal)} of {img.shape[0]} envs byte-identical to their state's image from the batch of {len(STATES)}")
    for j in unequal[:8]:
        d = (img[j] != small[j % len(STATES)]).any(-1)
        print(f"  env {j} ({STATES[j % len(STATES)]}): {int(d.sum())} pixels differ, first at (camera, row, column) {tuple(np.argwhere(d)[0])}")
    assert not unequal, f"{what}: envs {unequal[:20]} differ from their state's image"


@pytest.mark.parametrize("N", BATCHES)
def test_band_counts_and_slot_reuse(world, N):
    """The same states replicated over N envs: k_vis_shadow runs over 8, 4, 2 and 1 bands of rows (16 in the batch of five), where one workgroup
    meets ever more of the scene's big triangles and flushes its queue mid-loop; with 3 N views k_vis_render's workgroups walk several views
    each through one scratch slot.  The map is an atomicMax of keys that do not depend on the bands and the image does not depend on the order
    of the tile lists, so every env's image equals its state's image from the batch of five byte for byte, smooth and flat."""
    sim = world.batch(N)
    try:
        for smooth in (True, False):
            assert_replicas_equal(world.render(sim, smooth), world.small_images(smooth), f"N = {N} {'smooth' if smooth else 'flat'}")
    finally:
        sim.close()


def test_other_output_forms_at_256_envs(world):
    """avsim_render_rgb_f32 gives u8 / 255 exactly (divided on the host in IEEE float32) and render_cam_major the env-major images permuted,
    each at N = 256 (one band, slots reused), both together too."""
    N, smooth = 256, True
    sim = world.batch(N)
    try:
        u8 = world.render(sim, smooth)
        assert_replicas_equal(u8, world.small_images(smooth), "N = 256 u8")
        cm = world.render(sim, smooth, cam_major=True)
        assert cm.shape == (len(RE.VIS_CAMS), N, H, W, 3) and np.array_equal(cm, u8.transpose(1, 0, 2, 3, 4))
        ids = np.array([sim.manifest["camera_names"].index(c) for c in RE.VIS_CAMS], dtype=np.int32)
        want = u8.transpose(0, 1, 4, 2, 3).astype(np.float32) / np.float32(255)
        for cam_major in (0, 1):
            sim.set_option("render_cam_major", cam_major)
            f32 = np.full((len(ids), N, 3, H, W) if cam_major else (N, len(ids), 3, H, W), -1.0, np.float32)
            sim.h.check(sim.h.L.avsim_render_rgb_f32(sim.h.h, ids.ctypes.data, len(ids), H, W, f32.ctypes.data))
            assert sim.visual_info()["overflow"] == 0
            assert np.array_equal(f32, want.transpose(1, 0, 2, 3, 4) if cam_major else want), f"render_rgb_f32, cam_major {cam_major}"
    finally:
        sim.close()


def test_no_stale_shadow_maps(world):
    """After a set_qpos that changes env 0 only (H0 -> H1's pose) env 0 shows H1 -- the bytes of env 1 -- and every other env's image stays
    as it was."""
    smooth = True
    sim = world.batch(len(STATES))
    try:
        before = world.render(sim, smooth)
        assert np.array_equal(before, world.small_images(smooth))
        q = np.stack([world.S[s] for s in STATES])
        q[0] = world.S["H1"]
        sim.set_qpos(q)
        after = world.render(sim, smooth)
        assert np.array_equal(after[1:], before[1:]), "an env whose state did not change shows another image"
        changed = (after[0] != before[0]).any(-1).sum(axis=(1, 2))
        print(f"env 0 after set_qpos: {changed.tolist()} pixels changed per camera")
        assert (changed > 0).all() and np.array_equal(after[0], before[1])
    finally:
        sim.close()
