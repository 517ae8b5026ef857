"""What a pixel shows: the label tables and the specification of avsim_render_labels (include/avsim.h).

avsim_render_labels runs avsim_render_depth's cast and keeps, per pixel, the collision geom that won it: labels[n][c][i][j] = table[g], or
table[ngeom] where the ray meets nothing.  A table is uint8 [ngeom + 1] (label_table):

  "geom"    table[g] = g, nothing = 255                     names: the manifest's geom_names
  "body"    table[g] = geom_body[g], nothing = 255          names: the manifest's body_names
  "class"   0 background; 1 table (the world body's geom of that name); 2 frame (every other geom of the world body); 3 left_arm,
            4 left_gripper, 5 right_arm, 6 right_gripper, 7 middle_arm -- the arm by the name prefix of the body's root ancestor
            (body_parent up to the world's child), a gripper a body of that tree whose name contains "gripper" or "finger" (the middle arm
            carries cameras, no gripper) --; from 8 on one class per remaining body in body order, named by the body (slot, stick, ...)

Invisible geoms (geom_visible 0: the pin spheres of the fingers) have an entry like the others and are never drawn.

drop: labels whose pixels get the FAR PLANE as their depth, the value of a ray that meets nothing -- avsim_point_cloud, avsim_voxel_grid and
avsim_virtual_views keep d < max_depth, so the dropped geoms leave a cloud, a grid or a view with no change to those calls.  The label image
always holds the true label.

cast_reference states in float64 numpy what the oracle's ray caster (oracle/orc_render.c) does per geom, in its order of operations: its
minimum over the geoms, cast to float32, is orc_render_depth's image bit for bit (tests/test_segment_host.py), and labels_reference is its
arg-min through a table.  The device casts in float32 from float32 poses, so its image is compared with this one through the sub-pixel
rule of tests/test_gpu_segment.py, not bit for bit."""
import math

import numpy as np

MAX_CAMERAS = 16
MAX_SIZE = 4096             # height and width of avsim_render_depth's and avsim_render_labels's images
MAX_GEOMS = 128             # BL_MAX: the geoms a bin's list holds
BACKGROUND = 255            # nothing, in the "geom" and "body" tables
FAR_PLANE = 30.0
FIXED_CLASSES = ["background", "table", "frame", "left_arm", "left_gripper", "right_arm", "right_gripper", "middle_arm"]
ROBOT_CLASSES = FIXED_CLASSES[3:]       # the usual drop list of a cloud
KINDS = ("geom", "body", "class")


def read_model(manifest):
    """{geom_body, body_parent}: what label_table reads of the committed model blob a manifest belongs to (models/<task>_<arms>arms.avm; the
    blob's directory, compiler/compile.py write_blob)."""
    import os
    import struct
    from .constants import MODEL_DIR
    prefix = "dc_" if manifest.get("variant") == "data_collection" else ""
    with open(os.path.join(MODEL_DIR, f"{prefix}{manifest['task']}_{manifest['num_arms']}arms.avm"), "rb") as f:
        b = f.read()
    assert b[:8] == b"AVSIMMDL"
    out = {}
    for i in range(struct.unpack_from("<II", b, 8)[1]):
        name, dt, nd, d0, d1, d2, d3, off, nb = struct.unpack_from("<32sII4IQQ", b, 16 + 72 * i)
        name = name.rstrip(b"\0").decode()
        if name in ("geom_body", "body_parent"):
            out[name] = np.frombuffer(b, dtype="<i4", count=nb // 4, offset=off).copy()
    return out


def _ints(model, key):
    return np.asarray(model[key]).reshape(-1).astype(np.int64)


def class_table(manifest, model):
    """(table uint8 [ngeom + 1], CLASS_NAMES) of kind "class" (the module's docstring has the scheme)."""
    bnames, gnames = manifest["body_names"], manifest["geom_names"]
    parent, gbody = _ints(model, "body_parent"), _ints(model, "geom_body")
    names = list(FIXED_CLASSES)
    body_class = np.zeros(len(bnames), dtype=np.int64)
    for b in range(1, len(bnames)):
        root = b
        while parent[root] > 0:
            root = int(parent[root])
        arm = next((a for a in ("left", "right", "middle") if bnames[root].startswith(a + "_")), None)
        if arm is None:
            body_class[b] = len(names)
            names.append(bnames[b])
        elif arm != "middle" and ("gripper" in bnames[b] or "finger" in bnames[b]):
            body_class[b] = names.index(arm + "_gripper")
        else:
            body_class[b] = names.index(arm + "_arm")
    if len(names) > BACKGROUND:
        raise ValueError("class table: more classes than a uint8 label holds")
    table = np.zeros(len(gbody) + 1, dtype=np.uint8)
    for g, b in enumerate(gbody):
        table[g] = body_class[b] if b > 0 else (1 if gnames[g] == "table" else 2)
    return table, names


def label_table(manifest, model, kind):
    """(table uint8 [ngeom + 1], names) of kind "geom", "body" or "class"; names[label] says what a label is (for "class": CLASS_NAMES).
    model: the arrays of the model blob (compiler.compile.read_blob), of which geom_body and body_parent are read."""
    gbody = _ints(model, "geom_body")
    if len(gbody) > MAX_GEOMS:
        raise ValueError(f"label table: {len(gbody)} geoms, more than {MAX_GEOMS}")
    if kind == "geom":
        return np.append(np.arange(len(gbody)), BACKGROUND).astype(np.uint8), list(manifest["geom_names"])
    if kind == "body":
        if gbody.max() >= BACKGROUND:
            raise ValueError("body table: more bodies than a uint8 label holds")
        return np.append(gbody, BACKGROUND).astype(np.uint8), list(manifest["body_names"])
    if kind == "class":
        return class_table(manifest, model)
    raise ValueError(f"label table kind {kind!r}: one of {KINDS} (or a table)")


def drop_flags(drop, names=None):
    """uint8 [256], 1 at every label of `drop` (label values, or names of `names`); None for an empty list."""
    drop = list(drop) if drop is not None else []
    if not drop:
        return None
    flags = np.zeros(256, dtype=np.uint8)
    for d in drop:
        if isinstance(d, str):
            if names is None or d not in names:
                raise ValueError(f"drop: no label named {d!r}" + ("" if names is None else f" among {names}"))
            d = names.index(d)
        if not 0 <= int(d) <= 255:
            raise ValueError(f"drop: label {d} outside 0..255")
        flags[int(d)] = 1
    return flags


def check_labels(ncam_model, ngeom, cam_ids, height, width, table=None, drop=None, depth=True, labels=True):
    """ValueError for what avsim_render_labels refuses (null cam_ids and misaligned device pointers aside), and for a table or a drop
    array of the wrong length, which the C call cannot see.  depth / labels: whether that output is asked for."""
    ids = [int(c) for c in cam_ids]
    if not 1 <= len(ids) <= MAX_CAMERAS:
        raise ValueError(f"render_labels: {len(ids)} cameras, outside 1..{MAX_CAMERAS}")
    if not (1 <= int(height) <= MAX_SIZE and 1 <= int(width) <= MAX_SIZE):
        raise ValueError(f"render_labels: image size {height} x {width} outside 1..{MAX_SIZE}")
    if any(c < 0 or c >= int(ncam_model) for c in ids):
        raise ValueError("render_labels: camera index out of range")
    if not depth and not labels:
        raise ValueError("render_labels: neither depth nor labels is asked for")
    if drop is not None and not depth:
        raise ValueError("render_labels: drop changes the depth image, which is not asked for")
    if int(ngeom) > MAX_GEOMS:
        raise ValueError(f"render_labels: {ngeom} geoms, more than {MAX_GEOMS}")
    if table is not None and (np.asarray(table).dtype != np.uint8 or np.asarray(table).shape != (int(ngeom) + 1,)):
        raise ValueError(f"render_labels: a table is uint8 [{int(ngeom) + 1}] (one entry per geom and one for nothing)")
    if drop is not None and (np.asarray(drop).dtype != np.uint8 or np.asarray(drop).shape != (256,)):
        raise ValueError("render_labels: drop is uint8 [256], a flag per label")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cast, in float64

def quat_to_mat(q):
    w, x, y, z = (float(v) for v in q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def camera_pose(model, xpos, xmat, cam):
    """(cam_pos [3], cam_mat [3, 3]): the world pose of camera `cam` from the body poses xpos [nbody, 3] / xmat [nbody, 3, 3], the sums in
    the oracle's order."""
    b = int(_ints(model, "cam_body")[cam])
    Rb, pb = np.asarray(xmat, dtype=np.float64).reshape(-1, 3, 3)[b], np.asarray(xpos, dtype=np.float64).reshape(-1, 3)[b]
    cp, Rl = np.asarray(model["cam_pos"], dtype=np.float64).reshape(-1, 3)[cam], quat_to_mat(np.asarray(model["cam_quat"]).reshape(-1, 4)[cam])
    pc = np.array([pb[i] + Rb[i, 0] * cp[0] + Rb[i, 1] * cp[1] + Rb[i, 2] * cp[2] for i in range(3)])
    Rc = np.array([[Rb[i, 0] * Rl[0, j] + Rb[i, 1] * Rl[1, j] + Rb[i, 2] * Rl[2, j] for j in range(3)] for i in range(3)])
    return pc, Rc


def _slab(lo, hi, ok, o, v, s):
    """The interval of o + t v inside |x| <= s on one axis, met with [lo, hi]; a ray along the slab is kept iff it starts inside."""
    par = v == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-s - o) / v, (s - o) / v
    ta, tb = np.where(ta > tb, tb, ta), np.where(ta > tb, ta, tb)
    ok = ok & np.where(par, abs(o) <= s, True)
    return np.where(~par & (ta > lo), ta, lo), np.where(~par & (tb < hi), tb, hi), ok


def _disc(lo, hi, ok, a, b, c):
    """The roots of a t^2 + 2 b t + c = 0 (a > 0) as the interval of a sphere or of a cylinder's side."""
    disc = b * b - a * c
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.where(disc < 0, 0.0, disc))
        return (-b - s) / a, (-b + s) / a, ok & ~(disc < 0)


def cast_reference(model, geom_xpos, geom_xmat, cam_pos, cam_mat, cam, H, W, rows=None, cols=None):
    """float64 [ngeom, H, W]: the entry depth (metres along the optical axis) of every visible geom along the ray of every pixel of the
    H x W image of camera `cam` (an index: its fovy), whose world pose is cam_pos / cam_mat (camera_pose); inf where the ray misses the
    geom, enters it nearer than the near plane (t0 >= znear is required: a geom that holds the camera is not seen, back faces are culled)
    or the geom is invisible.  Per type, oracle/orc_render.c ray_interval: sphere and cylinder side by the quadratic's roots, box and
    cylinder caps by slabs, a hull by its half spaces (n.v < 0 bounds the entry, n.v > 0 the exit, a ray in a plane is kept iff it
    runs inside).  rows / cols: the rows and columns of the image to cast (None: all) -- the rays do not depend on which are asked for --;
    the result is then [ngeom, len(rows), len(cols)]."""
    gtype, gvis, hpl = _ints(model, "geom_type"), _ints(model, "geom_visible"), _ints(model, "geom_hplane").reshape(-1, 2)
    gsize, planes = np.asarray(model["geom_size"], dtype=np.float64).reshape(-1, 3), np.asarray(model["hull_plane"], dtype=np.float64).reshape(-1, 4)
    gx, gm = np.asarray(geom_xpos, dtype=np.float64).reshape(-1, 3), np.asarray(geom_xmat, dtype=np.float64).reshape(-1, 3, 3)
    pc, Rc = np.asarray(cam_pos, dtype=np.float64), np.asarray(cam_mat, dtype=np.float64).reshape(3, 3)
    znear = float(np.asarray(model["cam_clip"]).reshape(-1)[0])
    scale = 2.0 * math.tan(0.5 * float(np.asarray(model["cam_fovy"]).reshape(-1)[cam]) * 3.14159265358979323846 / 180.0) / H
    rows, cols = np.arange(H) if rows is None else np.asarray(rows), np.arange(W) if cols is None else np.asarray(cols)
    dx = ((cols + 0.5 - 0.5 * W) * scale)[None, :]
    dy = (-(rows + 0.5 - 0.5 * H) * scale)[:, None]
    H, W = len(rows), len(cols)
    dw = [Rc[k, 0] * dx + Rc[k, 1] * dy + Rc[k, 2] * -1.0 for k in range(3)]
    out = np.full((len(gtype), H, W), np.inf)
    for g in range(len(gtype)):
        if not gvis[g]:
            continue
        Rg, rel = gm[g], pc - gx[g]
        o = [Rg[0, k] * rel[0] + Rg[1, k] * rel[1] + Rg[2, k] * rel[2] for k in range(3)]
        v = [Rg[0, k] * dw[0] + Rg[1, k] * dw[1] + Rg[2, k] * dw[2] for k in range(3)]
        sz = gsize[g]
        lo, hi, ok = np.full((H, W), -1e30), np.full((H, W), 1e30), np.ones((H, W), dtype=bool)
        if gtype[g] == 2:
            a, b = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], o[0] * v[0] + o[1] * v[1] + o[2] * v[2]
            lo, hi, ok = _disc(lo, hi, ok, a, b, o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - sz[0] * sz[0])
        elif gtype[g] == 6:
            for k in range(3):
                lo, hi, ok = _slab(lo, hi, ok, o[k], v[k], sz[k])
        elif gtype[g] == 5:
            a, b, c = v[0] * v[0] + v[1] * v[1], o[0] * v[0] + o[1] * v[1], o[0] * o[0] + o[1] * o[1] - sz[0] * sz[0]
            slo, shi, sok = _disc(lo, hi, ok, a, b, c)
            side = a > 0
            lo, hi, ok = np.where(side, slo, lo), np.where(side, shi, hi), np.where(side, sok, ok & ~(c > 0))
            lo, hi, ok = _slab(lo, hi, ok, o[2], v[2], sz[1])
        elif gtype[g] == 7:
            for n in planes[hpl[g, 0]:hpl[g, 0] + hpl[g, 1]]:
                nv, no = n[0] * v[0] + n[1] * v[1] + n[2] * v[2], n[3] - (n[0] * o[0] + n[1] * o[1] + n[2] * o[2])
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = no / nv
                ok = ok & ~((nv == 0) & (no < 0))
                lo, hi = np.where((nv < 0) & (t > lo), t, lo), np.where((nv > 0) & (t < hi), t, hi)
        else:
            continue
        out[g] = np.where(ok & ~(lo > hi) & (lo >= znear), lo, np.inf)
    return out


def depth_reference(cast, zfar=FAR_PLANE):
    """float32 [H, W]: the depth image of a cast -- the nearest entry below the far plane, the far plane where there is none."""
    best = cast.min(axis=0)
    return np.where(best < zfar, best, zfar).astype(np.float32)


def labels_reference(cast, table, zfar=FAR_PLANE):
    """uint8 [H, W]: table[g] of the geom with the nearest entry (the first of equals, as the oracle's loop keeps it), table[ngeom] where
    no entry is below the far plane."""
    table = np.asarray(table, dtype=np.uint8)
    g = cast.argmin(axis=0)
    return np.where(cast.min(axis=0) < zfar, table[g], table[len(cast)])
