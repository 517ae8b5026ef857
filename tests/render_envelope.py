"""Sub-pixel envelopes of the oracle's images, and the kinematic states the renderers are compared in (test infrastructure only).

The envelope of an H x W image is made from the oracle's image at K H x K W (K odd): the vertical field of view is fixed and the scale is
2 tan(fovy / 2) / H, so the centre of pixel (i, j) is the centre of high-resolution pixel (K i + K // 2, K j + K // 2), and its eight
neighbours there are the rays 1 / K pixel off the centre.  Per pixel (and channel) lo / hi are the minimum and maximum over that 3 x 3 block;
a pixel whose DEPTH spread over the block exceeds EDGE_SPREAD is an edge pixel, the others are interior.  A device pixel conforms when
lo - tol <= value <= hi + tol.  The rule (Tally): no interior pixel may fail; of the edge pixels at most one per image and at most one
per 10 000 compared pixels of a test function -- a surface narrower than 1 / K pixel can pass between the nine rays, nothing else can."""
import numpy as np

from test_oracle_physics import OBJ, model_dict

CAMS = ["zed_cam_left", "zed_cam_right", "wrist_cam_left", "wrist_cam_right", "overhead_cam", "worms_eye_cam"]
K_PROXY, K_VISUAL = 5, 3
EDGE_SPREAD = 1e-2                      # metres of depth over the 3 x 3 block above which a pixel is an edge pixel
TOL_DEPTH, TOL_PROXY, TOL_VISUAL = 1e-4, 1, 2
FAR = 30.0                              # cam_clip[1] of every model: what a ray that hits nothing returns
TILE_W, TILE_H = 32, 16                 # k_render_depth's tile, for the failure message


class Envelope:
    def __init__(self, lo, hi, edge, centre):
        self.lo, self.hi, self.edge, self.centre = lo, hi, edge, centre


def _minmax(hi_res, K, rows_per_pixel):
    """hi_res [n * rows_per_pixel, W * K, ...]: rows_per_pixel = K (whole image) or 3 (the three rows around each centre)."""
    c = K // 2
    n, Wk = hi_res.shape[0] // rows_per_pixel, hi_res.shape[1]
    b = hi_res.reshape((n, rows_per_pixel, Wk // K, K) + hi_res.shape[2:])
    if rows_per_pixel == K:
        b = b[:, c - 1:c + 2]
    b = b[:, :, :, c - 1:c + 2]
    return b.min(axis=(1, 3)), b.max(axis=(1, 3)), b[:, 1, :, 1]


def depth_envelope(e, cam, H, W, K=K_PROXY, rows=None):
    """Envelope of the depth image of `cam` in the oracle's current state.  rows = (row0, step, n): only those rows of the image."""
    c = K // 2
    if rows is None:
        hr = e.render_depth(cam, K * H, K * W).astype(np.float64)
        lo, hi, ctr = _minmax(hr, K, K)
        plain = e.render_depth(cam, H, W)
    else:
        r0, step, n = rows
        three = [e.render_depth_rows(cam, K * H, K * W, K * r0 + c + d, K * step, n) for d in (-1, 0, 1)]
        hr = np.stack(three, axis=1).reshape(3 * n, K * W).astype(np.float64)
        lo, hi, ctr = _minmax(hr, K, 3)
        plain = e.render_depth_rows(cam, H, W, r0, step, n)
    assert np.array_equal(ctr.astype(np.float32), plain), f"{cam} {H}x{W}: the centre samples are not the plain image"
    return Envelope(lo, hi, (hi - lo) > EDGE_SPREAD, ctr)


def proxy_envelope(e, cam, H, W, K=K_PROXY):
    """(colour envelope, depth envelope) of the proxy colour image: one pass of orc_render_rgb at K H x K W gives both."""
    rgb, dep = e.render_rgb(cam, K * H, K * W)
    lo, hi, ctr = _minmax(rgb.astype(np.int32), K, K)
    dlo, dhi, dctr = _minmax(dep.astype(np.float64), K, K)
    prgb, pdep = e.render_rgb(cam, H, W)
    assert np.array_equal(ctr, prgb) and np.array_equal(dctr.astype(np.float32), pdep), f"{cam} {H}x{W}: the centre samples are not the plain image"
    edge = (dhi - dlo) > EDGE_SPREAD
    return Envelope(lo, hi, edge, ctr), Envelope(dlo, dhi, edge, dctr)


def visual_envelope(e, cam, H, W, scene, smooth, K=K_VISUAL, plain=None):
    """Colour envelope of the visual-mesh image (orc_vis_render_sm; its depth is 0 where a ray sees the sky: the far plane here).
    plain: the oracle's H x W image when the caller has it already (the oracle is slow), else it is rendered for the centre check."""
    rgb, _, dep = e.render_visual(cam, K * H, K * W, scene, smooth=smooth)
    dep = np.where(dep > 0, dep, FAR)
    lo, hi, ctr = _minmax(rgb.astype(np.int32), K, K)
    dlo, dhi, _ = _minmax(dep, K, K)
    if plain is None:
        plain = e.render_visual(cam, H, W, scene, smooth=smooth)[0]
    assert np.array_equal(ctr, plain), f"{cam} {H}x{W}: the centre samples are not the plain image"
    return Envelope(lo, hi, (dhi - dlo) > EDGE_SPREAD, ctr)


def violations(value, env, tol):
    """(interior, edge): bool images of the pixels of `value` outside the envelope (any channel, for colour)."""
    v = value.astype(np.float64 if env.lo.dtype == np.float64 else np.int32)
    bad = (v < env.lo - tol) | (v > env.hi + tol)
    if bad.ndim == 3:
        bad = bad.any(-1)
    return bad & ~env.edge, bad & env.edge


def describe(value, env, bad, label, rows=None, limit=12):
    out = []
    for i, j in np.argwhere(bad)[:limit]:
        r = i if rows is None else rows[0] + i * rows[1]
        out.append(f"{label} pixel ({r}, {j}) tile ({r // TILE_H}, {j // TILE_W}): device {value[i, j]} envelope [{env.lo[i, j]}, {env.hi[i, j]}]"
                   f" centre {env.centre[i, j]} {'edge' if env.edge[i, j] else 'interior'}")
    if bad.sum() > limit:
        out.append(f"{label}: ... {int(bad.sum())} pixels in all")
    return out


class Tally:
    """The rule over one test function: add() every image, then done()."""

    def __init__(self, interior_allowed=0):
        self.compared = self.interior = self.edge = 0
        self.interior_allowed = interior_allowed       # per image (visual meshes only: see tests/test_gpu_render_envelope.py)
        self.lines, self.failed = [], False

    def add(self, value, env, tol, label, rows=None):
        assert value.shape == env.lo.shape, (label, value.shape, env.lo.shape)
        bi, be = violations(value, env, tol)
        ni, ne = int(bi.sum()), int(be.sum())
        self.compared += bi.size
        self.interior += ni
        self.edge += ne
        if ni > self.interior_allowed or ne > 1:
            self.failed = True
        if ni or ne:
            self.lines += describe(value, env, bi | be, label, rows)
        return ni, ne

    def ok(self):
        return not self.failed and self.edge * 10000 <= self.compared

    def done(self):
        if self.lines:
            print("\n".join(self.lines))
        assert self.ok(), (f"{self.interior} interior and {self.edge} edge pixels outside the envelope in {self.compared} compared pixels "
                           f"(allowed: {self.interior_allowed} interior per image; edge 1 per image and 1 per 10 000 in all)\n" + "\n".join(self.lines))


# ---------------------------------------------------------------------------------------------------------------------------------------
# states

def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def mat_to_quat(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix."""
    t = np.trace(R)
    if t > 0:
        s = 2 * np.sqrt(1 + t)
        q = [s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i], q[1 + j], q[1 + k] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def rot(axis, angle):
    a = np.zeros(3)
    a[axis] = 1.0
    return quat_to_mat(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a]))


def cam_frame(md, e, name):
    """World position, rotation (columns: right, up, backwards) and tan(fovy / 2) of a camera in the oracle's current state."""
    ci = e.man["camera_names"].index(name)
    b = int(md["cam_body"][ci])
    Rb = e.arr("xmat", 9 * md["nbody"]).reshape(-1, 3, 3)[b]
    pb = e.arr("xpos", 3 * md["nbody"]).reshape(-1, 3)[b]
    return pb + Rb @ md["cam_pos"][ci], Rb @ quat_to_mat(md["cam_quat"][ci]), float(np.tan(np.radians(md["cam_fovy"][ci]) / 2))


def body_pose_for_geom(md, e, geom, centre, Rg):
    """Free-joint qpos (7) of the geom's body that puts the geom's centre at `centre` with orientation Rg."""
    g = e.man["geom_names"].index(geom)
    Rb = Rg @ quat_to_mat(md["geom_quat"].reshape(-1, 4)[g]).T
    return np.concatenate([centre - Rb @ md["geom_pos"].reshape(-1, 3)[g], mat_to_quat(Rb)])


def geom_vertex_depths(md, e, geom, cam):
    """Depths along the camera's optical axis of the eight corners of a box geom (of the bounding box of a cylinder / sphere)."""
    g = e.man["geom_names"].index(geom)
    sz = md["geom_size"].reshape(-1, 3)[g].copy()
    t = int(md["geom_type"][g])
    if t == 2:
        sz[:] = sz[0]
    elif t == 5:
        sz[:] = (sz[0], sz[0], sz[1])
    ng = len(e.man["geom_names"])
    p, R = e.arr("geom_xpos", 3 * ng).reshape(-1, 3)[g], e.arr("geom_xmat", 9 * ng).reshape(-1, 3, 3)[g]
    pc, Rc, _ = cam_frame(md, e, cam)
    corners = np.array([[sx, sy, sz_] for sx in (-1, 1) for sy in (-1, 1) for sz_ in (-1, 1)]) * sz
    return -((p + corners @ R.T - pc) @ Rc)[:, 2]


def coverage(e, q, adr, cam, H=60, W=80):
    """Share of the camera's H x W oracle depth image that the object whose free joint is at qpos[adr] changes (the image with the object
    against the image with it 100 m away); leaves the oracle at q."""
    away = q.copy()
    away[adr:adr + 3] += 100.0
    e.set_qpos(away)
    without = e.render_depth(cam, H, W)
    e.set_qpos(q)
    return float((e.render_depth(cam, H, W) != without).mean())


def in_front_of(md, e, q, cam, geom, adr, depth, off_right, off_up, tilt):
    """qpos with `geom` (long axis: x of a box, z of a cylinder) laid along the optical axis of `cam`, its centre `depth` in front of the
    camera and (off_right, off_up) off the axis, then turned by tilt = (about the camera's right, up and viewing axes)."""
    e.set_qpos(q)
    pc, Rc, _ = cam_frame(md, e, cam)
    g = e.man["geom_names"].index(geom)
    fwd = -Rc[:, 2]
    if int(md["geom_type"][g]) == 5:
        Rg = Rc.copy()                                             # the cylinder's axis (z) along the camera's z
    else:
        Rg = np.stack([fwd, Rc[:, 0], np.cross(fwd, Rc[:, 0])], axis=1)
    Rt = Rc @ rot(0, tilt[0]) @ rot(1, tilt[1]) @ rot(2, tilt[2]) @ Rc.T      # a rotation given in the camera's axes
    q = q.copy()
    q[adr:adr + 7] = body_pose_for_geom(md, e, geom, pc + depth * fwd + off_right * Rc[:, 0] + off_up * Rc[:, 1], Rt @ Rg)
    return q


def crosses_near_plane(md, e, q, cam, geom, adr, min_cover):
    e.set_qpos(q)
    d = geom_vertex_depths(md, e, geom, cam)
    znear = float(md["cam_clip"][0])
    assert d.min() < znear < d.max(), f"{geom} does not cross the near plane of {cam}: vertex depths {d.min():.3f} .. {d.max():.3f}"
    c = coverage(e, q, adr, cam)
    assert c >= min_cover, f"{geom} covers {c:.3f} of {cam}, less than {min_cover}"
    return c


def frame_bars_in_view(md, e, cam, depth):
    """[(geom, angle against the image rows in degrees, length in pixels)] of the frame's bars (the world body's elongated hulls) as the
    camera's oracle depth image `depth` shows them: the stretch of the bar's axis between its first and last unoccluded sample."""
    H, W = depth.shape
    names, ng = e.man["geom_names"], len(e.man["geom_names"])
    gx, gm = e.arr("geom_xpos", 3 * ng).reshape(-1, 3), e.arr("geom_xmat", 9 * ng).reshape(-1, 3, 3)
    hv, gh = md["hull_vert"].reshape(-1, 3), md["geom_hull"].reshape(-1, 2)
    pc, Rc, th = cam_frame(md, e, cam)
    out = []
    for g in range(ng):
        if md["geom_body"][g] != 0 or names[g] == "table" or gh[g, 1] < 4:
            continue
        v = gx[g] + hv[gh[g, 0]:gh[g, 0] + gh[g, 1]] @ gm[g].T
        c = v.mean(0)
        _, s, vt = np.linalg.svd(v - c)
        if s[1] > 0.3 * s[0]:
            continue                                    # a bracket or a plate, not a bar
        t = (v - c) @ vt[0]
        pts = (c + np.linspace(t.min(), t.max(), 41)[:, None] * vt[0] - pc) @ Rc
        seen = []
        for x, y, z in pts:
            z = -z
            if z > md["cam_clip"][0]:
                col, row = x / z / (2 * th / H) + W / 2, -y / z / (2 * th / H) + H / 2
                if 0 <= col < W and 0 <= row < H and abs(depth[int(row), int(col)] - z) < 0.04:
                    seen.append((row, col))
        if len(seen) >= 3:
            dr, dc = abs(seen[-1][0] - seen[0][0]), abs(seen[-1][1] - seen[0][1])
            out.append((g, float(np.degrees(np.arctan2(dr, dc))), float(np.hypot(dr, dc))))
    return out


def home_q(md, obj):
    q = md["qpos_home"].copy()
    a = int(md["objects_qposadr"][0])
    q[a:a + 7 * len(obj)] = np.asarray(obj, dtype=np.float64).reshape(-1)
    return q


def slot_states(e):
    """{name: qpos} of S0 .. S5 for slot_insertion with three arms; e: an OrcEnv of that model (left in state S5).  Every state's defining
    property is asserted here, on the oracle."""
    from test_gpu_physics import actions_wiggle
    md = model_dict()
    SLOT, STICK = 23, 30
    S = {}
    S["S0"] = home_q(md, OBJ)
    # S1: six wiggle steps of the oracle (Newton); both sides are then put into that qpos
    e.d.solver = 1
    e.reset(OBJ)
    for a in actions_wiggle(md, 6):
        e.env_step(a)
    S["S1"] = e.qpos.copy()
    assert np.abs(S["S1"][:23] - S["S0"][:23]).max() > 0.02
    # S2: the stick along the optical axis of wrist_cam_right, below the axis so that the camera looks along its top face, through the near plane
    S["S2"] = in_front_of(md, e, S["S0"], "wrist_cam_right", "stick", STICK, 0.15, 0.004, -0.034, (0.03, 0.05, 0.1))
    crosses_near_plane(md, e, S["S2"], "wrist_cam_right", "stick", STICK, 0.10)
    # S3: the slot in front of wrist_cam_left, turned about all three axes
    S["S3"] = in_front_of(md, e, S["S0"], "wrist_cam_left", "slot-1", SLOT, 0.09, -0.03, -0.03, (0.25, -0.3, 0.4))
    crosses_near_plane(md, e, S["S3"], "wrist_cam_left", "slot-1", SLOT, 0.10)
    # S4: the active-vision arm lowered and pitched up until the ZED cameras look across the table at a grazing angle, rolled so that the
    # frame's bars run diagonally through the image
    q = S["S0"].copy()
    q[16:22] += [0.8, 0.8, 0.8, 0.0, -1.9, 0.7]
    S["S4"] = q
    e.set_qpos(q)
    for cam in ("zed_cam_left", "zed_cam_right"):
        pc, Rc, th = cam_frame(md, e, cam)
        elev, roll = np.degrees(np.arcsin(-Rc[2, 2])), np.degrees(np.arcsin(abs(Rc[2, 0])))
        assert -15 < elev < -3, f"{cam} looks {elev:.1f} deg above the horizon"
        assert 20 < roll < 70, f"{cam} is rolled by {roll:.1f} deg"
        d = e.render_depth(cam, 60, 80)
        seen = d[d < FAR]
        assert seen.size > 0.3 * d.size and seen.max() / seen.min() >= 5, f"{cam}: depth {seen.min():.3f} .. {seen.max():.3f}"
        bars = [b for b in frame_bars_in_view(md, e, cam, d) if 20 <= b[1] <= 70 and b[2] >= 20]
        assert len(bars) >= 2, f"{cam}: bars of the frame that run diagonally through the image: {bars}"
    # S5: the stick across the top of overhead_cam's image, cut by the border in both upper corners; the camera's centre inside the slot's
    # first bar (the second one behind the camera): back faces are culled, the oracle does not show the slot
    q = S["S0"].copy()
    e.set_qpos(q)
    pc, Rc, th = cam_frame(md, e, "overhead_cam")
    fwd = -Rc[:, 2]
    Rg = Rc @ rot(2, 0.04) @ rot(0, 0.3)         # the stick's long axis along the image rows
    q[STICK:STICK + 7] = body_pose_for_geom(md, e, "stick", pc + 0.2 * (fwd + 0.93 * th * Rc[:, 1]), Rg)
    Rs = np.stack([Rc[:, 0], fwd, np.cross(Rc[:, 0], fwd)], axis=1)                           # the slot's y (from bar 2 to bar 1) forwards
    q[SLOT:SLOT + 7] = body_pose_for_geom(md, e, "slot-1", pc + np.array([0.01, 0.003, -0.004]), Rs @ rot(0, 0.2) @ rot(2, 0.3))
    S["S5"] = q
    e.set_qpos(q)
    ng = len(e.man["geom_names"])
    g = e.man["geom_names"].index("slot-1")
    local = (pc - e.arr("geom_xpos", 3 * ng).reshape(-1, 3)[g]) @ e.arr("geom_xmat", 9 * ng).reshape(-1, 3, 3)[g]
    assert (np.abs(local) < md["geom_size"].reshape(-1, 3)[g] - 1e-3).all(), "overhead_cam is not inside slot-1"
    with_slot = e.render_depth("overhead_cam", 60, 80)
    assert coverage(e, q, SLOT, "overhead_cam") == 0.0, "the oracle shows a geom that contains the camera"
    no_stick = q.copy()
    no_stick[STICK:STICK + 3] += 100.0
    e.set_qpos(no_stick)
    changed = e.render_depth("overhead_cam", 60, 80) != with_slot
    e.set_qpos(q)
    assert changed[0, 0] and changed[0, 79] and not changed[59].any() and 0.03 < changed.mean() < 0.5, "the stick is not cut by both upper corners"
    return S


def other_task_states(task, e):
    """{name: qpos}: the reset pose and the task's round object (hook: a cylinder; tube_transfer: the ball) in front of wrist_cam_right,
    across its near plane."""
    md = model_dict(task)
    a0 = int(md["objects_qposadr"][0])
    home = md["qpos_home"].copy()
    S = {"R0": home}
    if task == "hook_package":
        S["R2"] = in_front_of(md, e, home, "wrist_cam_right", "hook", a0, 0.09, 0.002, -0.012, (0.06, -0.04, 0.0))
        crosses_near_plane(md, e, S["R2"], "wrist_cam_right", "hook", a0, 0.03)
    else:
        assert task == "tube_transfer"
        S["R2"] = in_front_of(md, e, home, "wrist_cam_right", "ball", a0, 0.033, 0.003, -0.002, (0.0, 0.0, 0.0))
        crosses_near_plane(md, e, S["R2"], "wrist_cam_right", "ball", a0, 0.01)
    return S


def scene_of(task, arms):
    """The expanded visual scene OrcEnv.render_visual takes (compiler/vismesh.py over the mesh library and the model blob)."""
    import os
    from av_aloha_amd.compiler import vismesh
    from av_aloha_amd.compiler.compile import read_blob
    from test_oracle_physics import ROOT
    lib = read_blob(os.path.join(ROOT, "models", "visual_meshes.avv"))
    mdl = read_blob(os.path.join(ROOT, "models", f"{task}_{arms}arms.avm"))
    return vismesh.expand_instances(lib, mdl) + (lib["lib_tex"],)


VIS_HW = (40, 56)
VIS_CAMS = ["overhead_cam", "wrist_cam_right", "zed_cam_left"]
NOISE_DEVICE = 1e-6         # the order of the device's f32 pose error (tests/test_gpu_pointcloud.py bounds it at 1e-5)


def visual_reference(md, e, scene, q, cam, smooth, seed=0):
    """(envelope of the visual-mesh image of state q, the oracle's own image of q disturbed by NOISE_DEVICE, its (interior, edge) counts
    of pixels outside the envelope): what the reference alone does under the device's pose error."""
    H, W = VIS_HW
    e.set_qpos(q)
    env = visual_envelope(e, cam, H, W, scene, smooth, plain=None)
    e.set_qpos(disturbed(md, q, NOISE_DEVICE, np.random.default_rng(seed)))
    img = e.render_visual(cam, H, W, scene, smooth=smooth)[0]
    e.set_qpos(q)
    bi, be = violations(img, env, TOL_VISUAL)
    return env, img, (int(bi.sum()), int(be.sum()))


def disturbed(md, q, sigma, rng):
    """q with all 23 arm joints and every object's position disturbed by Gaussian noise of `sigma` (rad, m)."""
    q = q.copy()
    q[:23] += sigma * rng.standard_normal(23)
    for a in md["objects_qposadr"]:
        q[int(a):int(a) + 3] += sigma * rng.standard_normal(3)
    return q


# ---------------------------------------------------------------------------------------------------------------------------------------
# the default image of the facades: shadows 1, samples 4 (DESIGN.md "The renderer's shadow contract"; the model: oracle/orc_vis.c
# orc_vis_render_model)

SHADOW_SIZE = 512                       # option "render_shadow_size": the default
POSE_BOUND = 1e-5                       # metres: what tests/test_gpu_pointcloud.py bounds the device's pose error by (NOISE_DEVICE is its order)
FRAGILE_MARGIN = 2.0
SHIFTS = (-0.2, 0.0, 0.2)               # pixel: the 0.2-pixel rule of the one-ray images (K = 5 there: the rays 1 / 5 pixel off the centre)


def light_box(md):
    """(half extent in metres, texels per metre at `shn` = 1) of the light's shadow box."""
    half = float(md["render_light"][3])
    return half, 1.0 / (2.0 * half)


def fragile_bounds(md, shn, margin=FRAGILE_MARGIN):
    """(eps in texels, delta in metres) of the model's fragile verdicts.

    A verdict compares the map's value at the texel that holds the sample's light-plane position with the sample's height.  The device's
    poses are off the oracle's by at most POSE_BOUND = 1e-5 m (NOISE_DEVICE = 1e-6 is the order, tests/test_gpu_pointcloud.py holds the bound):
    that moves the position by up to POSE_BOUND x itex texels (0.0043 texel at 512) and a height by up to POSE_BOUND.  Receiver and occluder
    move independently, so eps and delta are FRAGILE_MARGIN = 2 times those figures: eps = 2e-5 m x itex (0.0085 texel at 512, 0.034 at
    2048), delta = 2e-5 m.

    Measured (test_render_envelope_host.py::test_non_fragile_verdicts_survive_pose_noise: visual_reference's noise scheme, NOISE_DEVICE, seed
    0, every shadow state, the three cameras, smooth and flat): of 31 048 verdicts 18 are fragile at margin 2 and 0 of the others flipped (the flip
    count the margin has to reach: 0); margins 0.5 and 1 flip none either, with 3 and 10 fragile: the noise of this seed is smaller than the
    bound the margin is derived from."""
    return margin * POSE_BOUND * shn * light_box(md)[1], margin * POSE_BOUND


def model_renders(md, e, cam, H, W, scene, smooth, shn, shmap=None, shifts=SHIFTS, **kw):
    """The model's renders of the oracle's current state over the shifted sampling patterns (shmap: another state's map for a counter-image)."""
    eps, delta = fragile_bounds(md, shn)
    if shmap is None:
        shmap = e.shadow_map(scene, shn)
    return [e.render_model(cam, H, W, scene, smooth, shmap, dx=dx, dy=dy, eps_tex=eps, delta=delta, **kw) for dy in shifts for dx in shifts]


def production_envelope(e, cam, H, W, scene, smooth, shn=SHADOW_SIZE, md=None):
    """Envelope of the image with shadows 1, samples 4: per channel the minimum and the maximum over the nine model renders with ss = 2 whose
    sampling pattern is shifted by (dx, dy) in {-0.2, 0, +0.2}^2 pixel; a fragile sample enters with its shadowed and with its lit colour.
    Edge pixels: the depth of the 36 samples (sky: the far plane) spreads by more than EDGE_SPREAD.  The envelope also carries .shadowed and
    .fragile, bool images of the unshifted render (a fragment of the pixel is shadowed / has a fragile verdict)."""
    md = md or model_dict()
    rs = model_renders(md, e, cam, H, W, scene, smooth, shn)
    lo = np.min([r["lo"] for r in rs], axis=0).astype(np.int32)
    hi = np.max([r["hi"] for r in rs], axis=0).astype(np.int32)
    far = lambda d: np.where(d > 0, d, FAR)
    dlo = np.min([np.minimum(far(r["dmin"]), far(r["dmax"])) for r in rs], axis=0)
    dhi = np.max([np.maximum(far(r["dmin"]), far(r["dmax"])) for r in rs], axis=0)
    env = Envelope(lo, hi, (dhi - dlo) > EDGE_SPREAD, rs[4]["rgb"].astype(np.int32))
    env.shadowed, env.fragile = (rs[4]["flag"] & 1).astype(bool), (rs[4]["flag"] & 2).astype(bool)
    return env


def production_reference(md, e, scene, q, cam, smooth, shn=SHADOW_SIZE, seed=0):
    """visual_reference for the default image: (envelope of state q, the model's own image of q disturbed by NOISE_DEVICE, its (interior,
    edge) counts outside the envelope)."""
    H, W = VIS_HW
    e.set_qpos(q)
    env = production_envelope(e, cam, H, W, scene, smooth, shn, md)
    e.set_qpos(disturbed(md, q, NOISE_DEVICE, np.random.default_rng(seed)))
    img = e.render_model(cam, H, W, scene, smooth, e.shadow_map(scene, shn))["rgb"]
    e.set_qpos(q)
    bi, be = violations(img, env, TOL_VISUAL)
    return env, img, (int(bi.sum()), int(be.sum()))


def verdict_flips(md, e, scene, q, cam, smooth, shn=SHADOW_SIZE, margin=FRAGILE_MARGIN, seed=0):
    """(verdicts compared, of them fragile, non-fragile ones flipped) between the model of state q and of q disturbed by NOISE_DEVICE: the
    fragments that both images look up in the map at the same sample of the same triangle."""
    H, W = VIS_HW
    eps, delta = fragile_bounds(md, shn, margin)
    e.set_qpos(q)
    a = e.render_model(cam, H, W, scene, smooth, e.shadow_map(scene, shn), eps_tex=eps, delta=delta)
    e.set_qpos(disturbed(md, q, NOISE_DEVICE, np.random.default_rng(seed)))
    b = e.render_model(cam, H, W, scene, smooth, e.shadow_map(scene, shn))
    e.set_qpos(q)
    both = ((a["sflag"] & 4) != 0) & ((b["sflag"] & 4) != 0) & (a["tri"] == b["tri"])
    fragile = both & ((a["sflag"] & 2) != 0)
    flipped = both & ~fragile & ((a["sflag"] & 1) != (b["sflag"] & 1))
    return int(both.sum()), int(fragile.sum()), int(flipped.sum())


SHADOW_STATES = ["H0", "H1", "H2", "H3", "H4"]
MIN_SHADOWED, MAX_FRAGILE = 0.02, 0.01       # of an image's pixels: the overhead image's shadowed ones, any image's fragile ones


def shadow_states(e, scene=None):
    """{name: qpos} of the states the default image is compared in (slot_insertion, three arms; the light shines straight down):
    H0 the reset pose; H1 the stick 5 cm above the slot, turned against it: a detached shadow on the slot and the table; H2 the left gripper
    low over the stick, the slot under the forearm: the arm's shadow across both; H3 the stick rolled by 45 deg about its long axis and
    resting on one edge: under the overhang the gap to the table goes to zero, a contact shadow thinner than the bias; H4 the slot on the
    table across the border x = +0.6 m of the light's box (the table ends at 0.61 m, overhead_cam sees 0.65 m) and the stick 5 cm above it
    along the border: the shadow ends where the box does.  H1, H3 and H4 also turn the right arm (which carries wrist_cam_right) by a state's own
    angle, so that no two envs of a batch share an arm pose.
    With `scene`, every state's two conditions are asserted on the model and the figures returned too: (states, {name: (share of
    overhead_cam's pixels shadowed, largest share of fragile pixels over VIS_CAMS)})."""
    md = model_dict()
    SLOT, STICK = 23, 30
    S = {"H0": home_q(md, OBJ)}
    e.set_qpos(S["H0"])
    ng = len(e.man["geom_names"])
    gx = lambda name: e.arr("geom_xpos", 3 * ng).reshape(-1, 3)[e.man["geom_names"].index(name)].copy()
    gsz = lambda name: md["geom_size"].reshape(-1, 3)[e.man["geom_names"].index(name)]
    table_top = gx("table")[2] + gsz("table")[2]
    slot_top = gx("slot-1")[2] + gsz("slot-1")[2]
    hs = gsz("stick")
    # H1
    q = S["H0"].copy()
    q[8] += 0.15
    q[STICK:STICK + 7] = body_pose_for_geom(md, e, "stick", np.array([0.02, 0.13, slot_top + 0.05 + hs[2]]), rot(2, 0.5))
    S["H1"] = q
    # H2: the left arm's shoulder and elbow lowered until the fingers are 3 .. 8 cm above the stick's top; stick and slot are as high as each
    # other, so they lie 5 cm apart (two coplanar top faces would swap under any noise)
    q = S["H0"].copy()
    q[1] += 0.55
    q[2] -= 0.25
    e.set_qpos(q)
    nb = md["nbody"]
    bx = lambda name: e.arr("xpos", 3 * nb).reshape(-1, 3)[e.man["body_names"].index(name)].copy()
    grip, fore = bx("left_gripper_base"), bx("left_lower_forearm_link")
    gap = bx("left_left_finger_link")[2] - (table_top + 2 * hs[2])
    assert 0.03 < gap < 0.08, f"the left fingers are {gap:.3f} m above the stick's top"
    q[STICK:STICK + 7] = body_pose_for_geom(md, e, "stick", np.array([grip[0] + 0.12, grip[1], table_top + hs[2] + 1e-3]), rot(2, 0.3))
    q[SLOT:SLOT + 7] = body_pose_for_geom(md, e, "slot-1", np.array([fore[0] - 0.03, fore[1], table_top + gsz("slot-1")[2] + 1e-3]), rot(2, 1.2))
    S["H2"] = q
    # H3
    q = S["H0"].copy()
    q[8] -= 0.2
    drop = (hs[1] + hs[2]) / np.sqrt(2.0)
    q[STICK:STICK + 7] = body_pose_for_geom(md, e, "stick", np.array([0.05, -0.08, table_top + drop]), rot(2, 0.35) @ rot(0, np.pi / 4))
    S["H3"] = q
    # H4
    half = light_box(md)[0]
    edge_x = float(md["render_light"][7]) + half
    q = S["H0"].copy()
    q[8:10] += (-0.1, 0.2)
    q[SLOT:SLOT + 7] = body_pose_for_geom(md, e, "slot-1", np.array([edge_x, -0.15, table_top + gsz("slot-1")[2] + 1e-3]), rot(2, 0.0))
    q[STICK:STICK + 7] = body_pose_for_geom(md, e, "stick", np.array([edge_x, -0.15, slot_top + 0.05 + hs[2]]), rot(2, np.pi / 2 + 0.15))
    S["H4"] = q
    e.set_qpos(q)
    pc, Rc, th = cam_frame(md, e, "overhead_cam")
    p = (np.array([edge_x, -0.15, table_top]) - pc) @ Rc
    col, row = p[0] / -p[2] / (2 * th / VIS_HW[0]) + VIS_HW[1] / 2, -p[1] / -p[2] / (2 * th / VIS_HW[0]) + VIS_HW[0] / 2
    assert 1 < col < VIS_HW[1] - 1 and 1 < row < VIS_HW[0] - 1, f"the border of the light's box is not in overhead_cam's image: pixel ({row:.1f}, {col:.1f})"
    if scene is None:
        return S
    facts = {}
    for name in SHADOW_STATES:
        e.set_qpos(S[name])
        shmap = e.shadow_map(scene, SHADOW_SIZE)
        eps, delta = fragile_bounds(md, SHADOW_SIZE)
        shadowed, fragile = 0.0, 0.0
        for cam in VIS_CAMS:
            r = e.render_model(cam, *VIS_HW, scene, True, shmap, eps_tex=eps, delta=delta)
            if cam == "overhead_cam":
                shadowed = float(((r["flag"] & 1) != 0).mean())
            fragile = max(fragile, float(((r["flag"] & 2) != 0).mean()))
        assert shadowed >= MIN_SHADOWED, f"{name}: the model shadows {100 * shadowed:.2f} % of overhead_cam's pixels"
        assert fragile <= MAX_FRAGILE, f"{name}: {100 * fragile:.2f} % of an image's pixels hold a fragile sample"
        facts[name] = (shadowed, fragile)
    return S, facts
