"""Point clouds from depth images: the float32 specification of avsim_point_cloud (include/avsim.h).

Three stages.  The camera poses come from the device (avsim_camera_poses: records of 16 floats -- world position pc[3], rotation Rc[9] row
major, camera frame to world, the camera looks along its -z, tan(fovy / 2), three zeros).  Given those, everything below is float32 with
every operation rounded on its own, and the device equals it bit for bit:

  deprojection   scale = 2 t / H; x = ((c + 0.5) - 0.5 W) scale, y = -(((r + 0.5) - 0.5 H) scale) -- the renderer's own pixel rays --; the
                 camera-frame point (x d, y d, -d); w[i] = ((pc[i] + Rc[i][0] X) + Rc[i][1] Y) + Rc[i][2] Z
  crop           a pixel is a candidate when d < max_depth and lo[i] <= w[i] <= hi[i] on the three axes (a NaN drops it); the candidates of
                 an env in the order (camera slot, row, column), M of them
  cap            with M > C = MAX_CANDIDATES those at the positions (i M) // C, i < C, are used (M' = C), otherwise all (M' = M)
  FPS            selection 0 is candidate 0; mind = +inf; after every selection s, mind[k] = min(mind[k], (dx dx + dy dy) + dz dz) with
                 dx = w[k] - w[s]; the next selection is the largest mind, the lowest position among equals.  With M' < P the rule itself
                 repeats candidate 0 (every mind is 0)

Outputs per env: xyz [P, 3], index [P] (the flat pixel slot H W + r W + c; -1 and zeros when M = 0) and count (M, min(M', P))."""
import numpy as np

MAX_CANDIDATES = 16384      # AVSIM_PC_MAX_CANDIDATES
MAX_POINTS = 4096
MAX_CAMERAS = 16
MAX_PIXELS = 1 << 24
POSE_WIDTH = 16
FAR_PLANE = 30.0            # what avsim_render_depth writes where a ray meets nothing: the model's far clip plane (50 x the extent 0.6), the default max_depth

F = np.float32


def check_point_cloud(ncam_model, cam_ids, height, width, bounds, max_depth, npoints):
    """ValueError for what avsim_point_cloud refuses (null pointers aside)."""
    ids = [int(c) for c in cam_ids]
    if not 1 <= len(ids) <= MAX_CAMERAS:
        raise ValueError(f"point_cloud: {len(ids)} cameras, outside 1..{MAX_CAMERAS}")
    if not 1 <= int(npoints) <= MAX_POINTS:
        raise ValueError(f"point_cloud: npoints {npoints} outside 1..{MAX_POINTS}")
    if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
        raise ValueError(f"point_cloud: image size {height} x {width} outside 1..65535")
    if len(ids) * int(height) * int(width) > MAX_PIXELS:
        raise ValueError("point_cloud: more than 2^24 pixels per env")
    md = F(max_depth)
    if not (np.isfinite(md) and md > 0):
        raise ValueError("point_cloud: max_depth is finite and > 0")
    b = np.asarray(bounds, dtype=np.float32).reshape(-1)
    if b.shape != (6,):
        raise ValueError("point_cloud: bounds are xlo ylo zlo xhi yhi zhi")
    if not np.all(np.isfinite(b)):
        raise ValueError("point_cloud: a bound that is not finite")
    if np.any(b[:3] > b[3:]):
        raise ValueError("point_cloud: a lower bound above its upper bound")
    if any(c < 0 or c >= int(ncam_model) for c in ids):
        raise ValueError("point_cloud: camera index out of range")


def pixel_rays(t, height, width):
    """(x [W], y [H]) float32: the ray of pixel (r, c) is (x[c], y[r], -1) in the camera frame; t = tan(fovy / 2) as the device holds it."""
    scale = (F(2.0) * F(t)) / F(height)
    x = ((np.arange(width, dtype=np.float32) + F(0.5)) - F(0.5) * F(width)) * scale
    y = -(((np.arange(height, dtype=np.float32) + F(0.5)) - F(0.5) * F(height)) * scale)
    return x, y


def deproject(pose, depth):
    """World points float32 [ncam, H, W, 3] of one env's depth images [ncam, H, W] under its pose records [ncam, 16]."""
    pose = np.asarray(pose, dtype=np.float32).reshape(-1, POSE_WIDTH)
    depth = np.asarray(depth, dtype=np.float32)
    ncam, H, W = depth.shape
    out = np.empty((ncam, H, W, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for s in range(ncam):
            pc, Rc = pose[s, :3], pose[s, 3:12].reshape(3, 3)
            x, y = pixel_rays(pose[s, 12], H, W)
            d = depth[s]
            X, Y, Z = x[None, :] * d, y[:, None] * d, -d
            for i in range(3):
                out[s, :, :, i] = ((pc[i] + Rc[i, 0] * X) + Rc[i, 1] * Y) + Rc[i, 2] * Z
    return out


def candidates(world, depth, bounds, max_depth):
    """The flat pixels (ascending: slot, row, column) that pass the depth limit and the inclusive box; a NaN anywhere drops the pixel."""
    b = np.asarray(bounds, dtype=np.float32).reshape(6)
    w = world.reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = np.asarray(depth, dtype=np.float32).reshape(-1) < F(max_depth)
        for i in range(3):
            ok &= (w[:, i] >= b[i]) & (w[:, i] <= b[3 + i])
    return np.nonzero(ok)[0].astype(np.int64)


def cap_positions(M, C=MAX_CANDIDATES):
    """The positions among M candidates that are used: all, or with M > C the C positions (i M) // C in integer arithmetic."""
    if M <= C:
        return np.arange(M, dtype=np.int64)
    return (np.arange(C, dtype=np.int64) * np.int64(M)) // np.int64(C)


def fps(points, npoints):
    """Positions int64 [npoints] of farthest point sampling over float32 points [M', 3], M' >= 1 (module docstring)."""
    w = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    sel = np.zeros(npoints, dtype=np.int64)
    mind = np.full(len(w), np.inf, dtype=np.float32)
    s = 0
    with np.errstate(over="ignore"):
        for p in range(1, npoints):
            dx, dy, dz = w[:, 0] - w[s, 0], w[:, 1] - w[s, 1], w[:, 2] - w[s, 2]
            mind = np.minimum(mind, (dx * dx + dy * dy) + dz * dz)
            s = int(np.argmax(mind))          # the first of equals: the lowest position
            sel[p] = s
            if mind[s] == 0:                  # every mind is 0: candidate 0 from here on, which sel already holds
                break
    return sel


def point_cloud_env(pose, depth, bounds, max_depth, npoints, max_candidates=MAX_CANDIDATES):
    """(xyz float32 [P, 3], index int32 [P], count int32 [2]) of one env."""
    world = deproject(pose, depth)
    cand = candidates(world, depth, bounds, max_depth)
    M = len(cand)
    xyz, index = np.zeros((npoints, 3), dtype=np.float32), np.full(npoints, -1, dtype=np.int32)
    if M == 0:
        return xyz, index, np.array([0, 0], dtype=np.int32)
    used = cand[cap_positions(M, max_candidates)]
    pts = world.reshape(-1, 3)[used]
    sel = fps(pts, npoints)
    return pts[sel].copy(), used[sel].astype(np.int32), np.array([M, min(len(used), npoints)], dtype=np.int32)


def point_cloud_reference(poses, depth, bounds, max_depth, npoints):
    """The specification of avsim_point_cloud: poses float32 [N, ncam, 16] (avsim_camera_poses), depth float32 [N, ncam, H, W] ->
    (xyz float32 [N, P, 3], index int32 [N, P], count int32 [N, 2])."""
    depth = np.asarray(depth, dtype=np.float32)
    N = depth.shape[0]
    poses = np.asarray(poses, dtype=np.float32).reshape(N, depth.shape[1], POSE_WIDTH)
    res = [point_cloud_env(poses[n], depth[n], bounds, max_depth, npoints) for n in range(N)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res])
