"""Virtual orthographic views of the depth cameras: the float32 specification of avsim_virtual_views (include/avsim.h).

What RVT and RVT-2 feed their 2-D transformer: the fused cloud of an env's depth cameras re-rendered into a handful of axis-aligned
orthographic images of the workspace box.  The points and the candidate rule are the point cloud's (pointcloud.deproject,
pointcloud.candidates: d < max_depth, the inclusive box, a NaN drops the pixel); there is no cap.  A call names 1..6 views (repeats
allowed), each a code 0..5 -- a proper, unmirrored look at the box lo, hi from outside, row 0 at the top of the image:

  code  name  seen from       column runs along  row runs along   dist
  0     +x    the hi-x face   y ascending        z descending     hi_x - w_x
  1     -x    the lo-x face   y descending       z descending     w_x - lo_x
  2     +y    the hi-y face   x descending       z descending     hi_y - w_y
  3     -y    the lo-y face   x ascending        z descending     w_y - lo_y
  4     +z    above           x ascending        y descending     hi_z - w_z
  5     -z    below           x ascending        y ascending      w_z - lo_z

Every view of a call is (VH, VW), each side 1..1024.  In float32 with every operation rounded on its own, for an image axis of n pixels
(VW for a column, VH for a row) along world axis k -- the voxel grid's cell formula:

  inv = F(n) / (hi_k - lo_k); u = (w_k - lo_k) inv; i = min(floor(u), n - 1) -- a point on hi goes to the last pixel --;
  ascending the pixel is i, descending n - 1 - i

With `radius` r (0..4) a candidate at (pr, pc) covers the pixels (pr + dr, pc + dc), |dr|, |dc| <= r, inside the image.  Its key in a view
is the UNSIGNED 64-BIT value (bits(dist) << 32) | slot: the float32 bit pattern of its dist -- non-negative inside the box, +0 on the face --
above its flat pixel slot s H W + r W + c < 2^24.  The winner of a virtual pixel is the smallest key among the candidates that cover it:
the nearest point and, among equals, the lowest slot.  A minimum does not depend on the order it is taken in, so the device's atomic
scatter equals this file, and itself, on every call.  Per env:

  out    float32 [nviews, VH, VW, 8]: 0..2 the winner's colour F(u8) F(1 / 255) (0 without a colour image), 3 its dist in metres, 4..6 its
         world point -- deproject's values for the winning slot, not the pixel's centre --, 7 1.0
  index  int32 [nviews, VH, VW]: the winning slot

and a pixel nothing covers is eight +0.0 and index -1."""
import numpy as np

from . import pointcloud as pc

MAX_CAMERAS = pc.MAX_CAMERAS
MAX_PIXELS = pc.MAX_PIXELS
MAX_VIEWS = 6               # AVSIM_VV_MAX_VIEWS
MAX_SIZE = 1024             # AVSIM_VV_MAX_SIZE
MAX_RADIUS = 4              # AVSIM_VV_MAX_RADIUS
CHANNELS = 8
VIEW_NAMES = ("+x", "-x", "+y", "-y", "+z", "-z")
# per code: (dist axis, dist from hi, column axis, column descending, row axis, row descending)
VIEW_AXES = ((0, True, 1, False, 2, True), (0, False, 1, True, 2, True), (1, True, 0, True, 2, True),
             (1, False, 0, False, 2, True), (2, True, 0, False, 1, True), (2, False, 0, False, 1, False))
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

F = np.float32


def view_codes(names_or_codes):
    """The codes of views given by name (VIEW_NAMES) or by code; a single name or code is one view.  ValueError for an unknown name (a code
    out of range is check_virtual_views's, and the library's, to refuse)."""
    if isinstance(names_or_codes, (str, int, np.integer)):
        names_or_codes = [names_or_codes]
    codes = []
    for v in names_or_codes:
        if isinstance(v, str):
            if v not in VIEW_NAMES:
                raise ValueError(f"virtual_views: view {v!r} is none of {VIEW_NAMES}")
            codes.append(VIEW_NAMES.index(v))
        else:
            if int(v) != v:
                raise ValueError(f"virtual_views: view {v!r} is a name or an integer code")
            codes.append(int(v))
    return tuple(codes)


def view_size(size):
    """(VH, VW) of `size`, an int (a square) or two ints."""
    s = np.asarray(size)
    if s.ndim == 0:
        s = np.repeat(s, 2)
    if s.shape != (2,) or not np.all(s == np.floor(s)):
        raise ValueError("virtual_views: size is an int or two ints (VH, VW)")
    return int(s[0]), int(s[1])


def pixel_scale(bounds, n):
    """(inv [3], pixel size [3]) float32 of the box for an image axis of n pixels."""
    b = np.asarray(bounds, dtype=np.float32).reshape(6)
    with np.errstate(all="ignore"):
        ext = b[3:] - b[:3]
        return F(n) / ext, ext / F(n)


def check_virtual_views(ncam_model, cam_ids, height, width, bounds, max_depth, views, size, radius):
    """ValueError for what avsim_virtual_views refuses (null pointers and the alignment of a device pointer aside)."""
    ids = [int(c) for c in cam_ids]
    if not 1 <= len(ids) <= MAX_CAMERAS:
        raise ValueError(f"virtual_views: {len(ids)} cameras, outside 1..{MAX_CAMERAS}")
    if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
        raise ValueError(f"virtual_views: image size {height} x {width} outside 1..65535")
    if len(ids) * int(height) * int(width) > MAX_PIXELS:
        raise ValueError("virtual_views: more than 2^24 pixels per env")
    codes = view_codes(views)
    if not 1 <= len(codes) <= MAX_VIEWS:
        raise ValueError(f"virtual_views: {len(codes)} views, outside 1..{MAX_VIEWS}")
    if not all(0 <= c <= 5 for c in codes):
        raise ValueError("virtual_views: a view code outside 0..5")
    vh, vw = view_size(size)
    if not (1 <= vh <= MAX_SIZE and 1 <= vw <= MAX_SIZE):
        raise ValueError(f"virtual_views: a view size outside 1..{MAX_SIZE}")
    if int(radius) != radius or not 0 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"virtual_views: radius {radius} outside 0..{MAX_RADIUS}")
    md = F(max_depth)
    if not (np.isfinite(md) and md > 0):
        raise ValueError("virtual_views: max_depth is finite and > 0")
    b = np.asarray(bounds, dtype=np.float32).reshape(-1)
    if b.shape != (6,):
        raise ValueError("virtual_views: bounds are xlo ylo zlo xhi yhi zhi")
    if not np.all(np.isfinite(b)):
        raise ValueError("virtual_views: a bound that is not finite")
    if not np.all(b[:3] < b[3:]):
        raise ValueError("virtual_views: a lower bound that is not below its upper bound")
    for n in (vh, vw):          # every axis against both image sides, whichever views are named
        inv, px = pixel_scale(b, n)
        if not (np.all(np.isfinite(inv)) and np.all(np.isfinite(px))):
            raise ValueError("virtual_views: an extent whose pixel size or its reciprocal is not a finite float32")
    if any(c < 0 or c >= int(ncam_model) for c in ids):
        raise ValueError("virtual_views: camera index out of range")


def pixels(w, lo, hi, n, descending):
    """int64 pixel of the float32 coordinates w on an image axis of n pixels over [lo, hi]."""
    inv = F(n) / (F(hi) - F(lo))
    u = (np.asarray(w, dtype=np.float32) - F(lo)) * inv
    i = np.minimum(np.floor(u), F(n) - F(1.0)).astype(np.int64)
    return (n - 1 - i) if descending else i


def view_keys(points, slots, bounds, code, size, radius):
    """uint64 [VH VW]: the smallest key per virtual pixel of view `code` over the candidates (float32 points [M, 3], their flat slots [M]);
    EMPTY where nothing covers the pixel."""
    vh, vw = size
    b = np.asarray(bounds, dtype=np.float32).reshape(6)
    w = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    da, from_hi, ca, cdesc, ra, rdesc = VIEW_AXES[code]
    dist = (b[3 + da] - w[:, da]) if from_hi else (w[:, da] - b[da])
    pcol = pixels(w[:, ca], b[ca], b[3 + ca], vw, cdesc)
    prow = pixels(w[:, ra], b[ra], b[3 + ra], vh, rdesc)
    key = (np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(slots).astype(np.uint64)
    keys = np.full(vh * vw, EMPTY, dtype=np.uint64)
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            r, c = prow + dr, pcol + dc
            m = (r >= 0) & (r < vh) & (c >= 0) & (c < vw)
            np.minimum.at(keys, r[m] * vw + c[m], key[m])
    return keys


def virtual_views_env(pose, depth, rgb, bounds, max_depth, views, size, radius):
    """(out float32 [nviews, VH, VW, 8], index int32 [nviews, VH, VW]) of one env: pose [ncam, 16], depth [ncam, H, W], rgb uint8
    [ncam, H, W, 3] or None."""
    codes, (vh, vw), radius = view_codes(views), view_size(size), int(radius)
    world = pc.deproject(pose, depth)
    cand = pc.candidates(world, depth, bounds, max_depth)
    flat = world.reshape(-1, 3)
    colour = None if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    out = np.zeros((len(codes), vh * vw, CHANNELS), dtype=np.float32)
    index = np.full((len(codes), vh * vw), -1, dtype=np.int32)
    for v, code in enumerate(codes):
        keys = view_keys(flat[cand], cand, bounds, code, (vh, vw), radius)
        hit = keys != EMPTY
        slot = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        if colour is not None:
            out[v, hit, 0:3] = colour[slot].astype(np.float32) * F(1.0 / 255.0)
        out[v, hit, 3] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out[v, hit, 4:7] = flat[slot]
        out[v, hit, 7] = F(1.0)
        index[v, hit] = slot.astype(np.int32)
    return out.reshape(len(codes), vh, vw, CHANNELS), index.reshape(len(codes), vh, vw)


def virtual_views_reference(poses, depth, rgb, bounds, max_depth, views, size, radius):
    """The specification of avsim_virtual_views: poses float32 [N, ncam, 16] (avsim_camera_poses), depth float32 [N, ncam, H, W], rgb uint8
    [N, ncam, H, W, 3] (avsim_render_rgb's env-major layout) or None -> (out float32 [N, nviews, VH, VW, 8], index int32 [N, nviews, VH, VW])."""
    depth = np.asarray(depth, dtype=np.float32)
    N = depth.shape[0]
    poses = np.asarray(poses, dtype=np.float32).reshape(N, depth.shape[1], pc.POSE_WIDTH)
    res = [virtual_views_env(poses[n], depth[n], None if rgb is None else rgb[n], bounds, max_depth, views, size, radius) for n in range(N)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
