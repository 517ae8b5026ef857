"""av_aloha_amd/segment.py on the CPU: the float64 cast that the label image is compared with equals the oracle's depth image bit for bit,
the tables of all ten committed models, the precondition of the GPU file's comparison rule, and check_labels's refusals."""
import json
import os

import numpy as np
import pytest

import render_envelope as RE
import segment_util as SU
from av_aloha_amd import segment
from av_aloha_amd.compiler.compile import read_blob
from orc_env import OrcEnv
from test_oracle_physics import ROOT, model_dict

H, W = 30, 40
TASKS = ["slot_insertion", "hook_package", "insert_peg", "sew_needle", "tube_transfer"]
MODELS = [(t, a) for t in TASKS for a in (2, 3)]


@pytest.fixture(scope="module")
def worlds():
    """task -> (model, oracle, states), made when first asked for; the states' defining properties are asserted while they are built."""
    made = {}

    def get(task):
        if task not in made:
            e = OrcEnv(task, 3)
            made[task] = (model_dict(task), e, SU.states_of(task, e))
        return made[task]
    yield get
    for _, e, _ in made.values():
        e.close()


def check_cast(md, e, q, cam, types):
    e.set_qpos(q)
    cast = SU.oracle_cast(md, e, cam, H, W)
    ref = e.render_depth(cam, H, W)
    got = segment.depth_reference(cast, float(md["cam_clip"][1]))
    assert got.dtype == np.float32 and np.array_equal(got, ref), f"{cam}: {(got != ref).sum()} of {ref.size} pixels differ from orc_render_depth, by up to {np.abs(got - ref).max()}"
    seen = {int(md["geom_type"][g]) for g in np.unique(cast.argmin(axis=0)[cast.min(axis=0) < RE.FAR])}
    assert types <= seen, f"{cam}: geom types seen {sorted(seen)}, wanted {sorted(types)}"
    # invisible geoms are never cast; the arg-min through the identity is the geom itself
    assert np.isinf(cast[np.asarray(md["geom_visible"]).reshape(-1) == 0]).all()
    table, _ = segment.label_table(e.man, md, "geom")
    lab = segment.labels_reference(cast, table)
    assert np.array_equal(lab == segment.BACKGROUND, ref == np.float32(RE.FAR))


@pytest.mark.parametrize("state", SU.HOST_SLOT)
def test_cast_equals_the_oracle_slot_insertion(worlds, state):
    """The minimum of cast_reference over the geoms, as float32, is OrcEnv.render_depth bit for bit: S0, S1, S2, S3, S5 x four cameras at
    30 x 40 (hulls and boxes, through the near plane in S2 / S3, the camera inside a box in S5)."""
    md, e, S = worlds("slot_insertion")
    for cam in SU.HOST_CAMS:
        check_cast(md, e, S[state], cam, {7} if cam != "zed_cam_left" else {6, 7})


@pytest.mark.parametrize("task,gtype", [("hook_package", 5), ("tube_transfer", 2)])
def test_cast_equals_the_oracle_round_geoms(worlds, task, gtype):
    """R2 of the other tasks: the hook's cylinder / the ball's sphere through the near plane of wrist_cam_right."""
    md, e, S = worlds(task)
    check_cast(md, e, S["R2"], "wrist_cam_right", {gtype})


@pytest.mark.parametrize("task,arms", MODELS)
def test_tables_of_every_committed_model(task, arms):
    man = json.load(open(os.path.join(ROOT, "models", f"{task}_{arms}arms.json")))
    md = read_blob(os.path.join(ROOT, "models", f"{task}_{arms}arms.avm"))
    gn, bn, gb = man["geom_names"], man["body_names"], np.asarray(md["geom_body"]).reshape(-1)
    ng = len(gn)
    geom, gnames = segment.label_table(man, md, "geom")
    assert geom.dtype == np.uint8 and np.array_equal(geom, list(range(ng)) + [255]) and gnames == gn
    body, bnames = segment.label_table(man, md, "body")
    assert body.dtype == np.uint8 and np.array_equal(body[:ng], gb) and body[ng] == 255 and bnames == bn
    cls, names = segment.label_table(man, md, "class")
    assert cls.dtype == np.uint8 and cls.shape == (ng + 1,) and names[:8] == segment.FIXED_CLASSES and len(set(names)) == len(names)
    # every geom has a class, the invisible ones too; nothing is class 0 but nothing
    assert cls[ng] == 0 and (cls[:ng] >= 1).all() and cls.max() < len(names)
    assert (np.asarray(md["geom_visible"]).reshape(-1) == 0).any()
    # known answers
    assert cls[gn.index("table")] == 1
    world = [g for g in range(ng) if gb[g] == 0 and gn[g] != "table"]
    assert world and all(cls[g] == 2 for g in world)
    assert names[cls[gn.index("left_left_finger")]] == "left_gripper" and names[cls[gn.index("right_right_finger")]] == "right_gripper"
    wrist3 = [g for g in range(ng) if bn[gb[g]] == "vx300s_7dof_wrist_3_link"]
    assert wrist3 and all(names[cls[g]] == "middle_arm" for g in wrist3)
    for g in range(ng):
        b = bn[gb[g]]
        if b.startswith(("left_", "right_")):
            side = b.split("_")[0]
            assert names[cls[g]] == side + ("_gripper" if "gripper" in b or "finger" in b else "_arm"), (gn[g], b)
    # the task's own bodies: one class each from 8 on, in body order, named by the body
    own = names[8:]
    assert own == [b for b in bn if b in own] and all(names[cls[g]] == bn[gb[g]] for g in range(ng) if cls[g] >= 8)
    if task == "slot_insertion":
        assert own == ["slot", "stick"]
        assert names[cls[gn.index("stick")]] == "stick" and names[cls[gn.index("slot-1")]] == "slot" and names[cls[gn.index("slot-2")]] == "slot"
    if task == "hook_package":
        assert own[:3] == ["wall", "hook", "package"]
    if task == "tube_transfer":
        assert own[:2] == ["ball", "tube1"]
    with pytest.raises(ValueError):
        segment.label_table(man, md, "link")


@pytest.mark.parametrize("task,states,env,cam", SU.CASES)
def test_most_pixels_have_one_accepted_label(worlds, task, states, env, cam):
    """The comparison rule's precondition at every (state, camera, size) tests/test_gpu_segment.py uses: at least 75 % of an image's
    pixels have exactly one accepted label, through the identity table (the finest one: a coarser table accepts no more labels)."""
    md, e, S = worlds(task)
    e.set_qpos(S[states[env]])
    table, _ = segment.label_table(e.man, md, "geom")
    for h, w in SU.SIZES:
        acc = SU.accepted(SU.nine_rays(md, e, cam, h, w), table)
        share = SU.single_share(acc)
        print(f"{task} {states[env]} {cam} {h}x{w}: {100 * share:.1f} % of the pixels have one accepted label")
        assert acc.any(axis=0).all()
        assert share >= SU.MIN_SINGLE


def test_nine_rays_are_the_high_resolution_image(worlds):
    """The sub-grid nine_rays casts is the 3 x 3 block around every pixel centre of the K H x K W cast, and its centre ray is the plain image's."""
    md, e, S = worlds("slot_insertion")
    e.set_qpos(S["S3"])
    K, c = SU.K, SU.K // 2
    rays = SU.nine_rays(md, e, "wrist_cam_left", 6, 9)
    full = SU.oracle_cast(md, e, "wrist_cam_left", K * 6, K * 9)
    block = full.reshape(len(full), 6, K, 9, K)[:, :, c - 1:c + 2, :, c - 1:c + 2]
    assert np.array_equal(rays, block)
    assert np.array_equal(rays[:, :, 1, :, 1], SU.oracle_cast(md, e, "wrist_cam_left", 6, 9))


def test_accepted_and_tally_rule():
    """The rule on a made-up cast of two geoms: a pixel both reach within the tolerance accepts both, a miss among the nine rays accepts
    the background, and the tally fails one wrong single-label pixel but allows one wrong pixel among those with several."""
    rays = np.full((2, 2, 3, 2, 3), np.inf)
    rays[0, 0, :, 0, :] = 1.0                       # pixel (0, 0): geom 0 alone
    rays[0, 0, :, 1, :] = 1.0
    rays[1, 0, 1, 1, 1] = 1.0 + 0.5 * RE.TOL_DEPTH  # pixel (0, 1): geom 1 within the tolerance at one ray
    rays[1, 1, :, 0, :] = 2.0                       # pixel (1, 0): geom 1, one ray misses
    rays[1, 1, 0, 0, 0] = np.inf
    table = np.array([3, 9, 0], dtype=np.uint8)
    acc = SU.accepted(rays, table)
    sets = [[np.flatnonzero(acc[:, i, j]).tolist() for j in range(2)] for i in range(2)]
    assert sets == [[[3], [3, 9]], [[0, 9], [0]]]
    t = SU.LabelTally()
    assert t.add(np.array([[3, 9], [0, 0]], dtype=np.uint8), acc, "good") == (0, 0)
    assert t.add(np.array([[3, 5], [0, 0]], dtype=np.uint8), acc, "one edge pixel") == (0, 1) and not t.failed
    with pytest.raises(AssertionError):
        t.done()                                    # one in eight compared, more than one per 10 000
    t = SU.LabelTally()
    assert t.add(np.array([[9, 3], [9, 0]], dtype=np.uint8), acc, "wrong single") == (1, 0) and t.failed


def test_drop_flags():
    names = segment.FIXED_CLASSES + ["slot", "stick"]
    f = segment.drop_flags(["left_arm", 9, "slot"], names)
    assert f.dtype == np.uint8 and f.shape == (256,) and np.flatnonzero(f).tolist() == [3, 8, 9]
    assert segment.drop_flags([], names) is None and segment.drop_flags(None) is None
    for bad in (["arm"], [256], [-1]):
        with pytest.raises(ValueError):
            segment.drop_flags(bad, names)
    with pytest.raises(ValueError):
        segment.drop_flags(["slot"])


def test_check_labels_refusals():
    table, drop = np.zeros(85, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    segment.check_labels(8, 84, [0, 2], 30, 40)
    segment.check_labels(8, 84, [7], 1, 4096, table, drop)
    segment.check_labels(8, 84, [0], 30, 40, table, None, depth=False)
    segment.check_labels(8, 84, [0], 30, 40, None, drop, labels=False)
    refused = [dict(cam_ids=[]), dict(cam_ids=list(range(8)) * 2 + [0]), dict(cam_ids=[8]), dict(cam_ids=[-1]), dict(height=0), dict(width=0),
               dict(height=4097), dict(width=4097), dict(depth=False, labels=False), dict(drop=drop, depth=False), dict(ngeom=129),
               dict(table=table[:84]), dict(table=table.astype(np.int32)), dict(drop=drop[:255]), dict(drop=drop.astype(bool))]
    for kw in refused:
        a = dict(ncam_model=8, ngeom=84, cam_ids=[0], height=30, width=40)
        a.update(kw)
        with pytest.raises(ValueError):
            segment.check_labels(**a)
