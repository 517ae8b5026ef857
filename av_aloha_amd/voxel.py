"""Voxel grids from depth images: the float32 specification of avsim_voxel_grid (include/avsim.h).

The points and the candidate rule are the point cloud's (pointcloud.deproject, pointcloud.candidates: d < max_depth, the inclusive box, a NaN
drops the pixel); there is no cap, every candidate counts.  For grid dims g = (gx, gy, gz) and the box lo, hi, per axis and in float32 with
every operation rounded on its own:

  inv = F(g) / (hi - lo), size = (hi - lo) / F(g)
  u = (w - lo) inv; i = min(floor(u), g - 1) -- a point on hi goes to the last cell --; frac = u - F(i); q = clip(int(frac 256), 0, 255)

A cell accumulates UNSIGNED 32-BIT INTEGERS: count, sum qx, sum qy, sum qz and, with a u8 colour image of the same pixels, sum r, sum g,
sum b.  Integer sums do not depend on the order of the adds, so the device's atomic scatter equals this file bit for bit; they cannot
overflow, at most MAX_PIXELS = 2^24 pixels per env times 255 being below 2^32.  A cell's eight float32 channels:

  0..2   the mean world position, lo + (F(i) + (F(sum q) / F(count) + 0.5) F(1 / 256)) size
  3..5   the mean colour, (F(sum c) / F(count)) F(1 / 255); 0 without a colour image
  6      F(count)
  7      occupancy, 1.0 or 0.0

and an empty cell is eight +0.0.  The layout is [N][gx][gy][gz][8]."""
import numpy as np

from . import pointcloud as pc

MAX_CAMERAS = pc.MAX_CAMERAS
MAX_PIXELS = pc.MAX_PIXELS
MAX_DIM = 256               # AVSIM_VOXEL_MAX_DIM
MAX_CELLS = 1 << 21         # AVSIM_VOXEL_MAX_CELLS: 128^3 and 100^3 fit
CHANNELS = 8

F = np.float32


def grid_dims(grid):
    """(gx, gy, gz) of `grid`, an int (a cube) or three ints."""
    g = np.asarray(grid)
    if g.ndim == 0:
        g = np.repeat(g, 3)
    if g.shape != (3,) or not np.all(g == np.floor(g)):
        raise ValueError("voxel_grid: grid is an int or three ints")
    return tuple(int(x) for x in g)


def cell_scale(bounds, grid):
    """(inv [3], size [3]) float32 of the box and the dims."""
    b = np.asarray(bounds, dtype=np.float32).reshape(6)
    g = np.array(grid, dtype=np.float32)
    with np.errstate(all="ignore"):
        ext = b[3:] - b[:3]
        return g / ext, ext / g


def check_voxel_grid(ncam_model, cam_ids, height, width, bounds, max_depth, grid):
    """ValueError for what avsim_voxel_grid refuses (null pointers aside)."""
    ids = [int(c) for c in cam_ids]
    if not 1 <= len(ids) <= MAX_CAMERAS:
        raise ValueError(f"voxel_grid: {len(ids)} cameras, outside 1..{MAX_CAMERAS}")
    if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
        raise ValueError(f"voxel_grid: image size {height} x {width} outside 1..65535")
    if len(ids) * int(height) * int(width) > MAX_PIXELS:
        raise ValueError("voxel_grid: more than 2^24 pixels per env")
    g = grid_dims(grid)
    if not all(1 <= x <= MAX_DIM for x in g):
        raise ValueError(f"voxel_grid: a grid dim outside 1..{MAX_DIM}")
    if g[0] * g[1] * g[2] > MAX_CELLS:
        raise ValueError("voxel_grid: more than 2^21 cells")
    md = F(max_depth)
    if not (np.isfinite(md) and md > 0):
        raise ValueError("voxel_grid: max_depth is finite and > 0")
    b = np.asarray(bounds, dtype=np.float32).reshape(-1)
    if b.shape != (6,):
        raise ValueError("voxel_grid: bounds are xlo ylo zlo xhi yhi zhi")
    if not np.all(np.isfinite(b)):
        raise ValueError("voxel_grid: a bound that is not finite")
    if not np.all(b[:3] < b[3:]):
        raise ValueError("voxel_grid: a lower bound that is not below its upper bound")
    inv, size = cell_scale(b, g)
    if not (np.all(np.isfinite(inv)) and np.all(np.isfinite(size))):
        raise ValueError("voxel_grid: an extent whose cell size or its reciprocal is not a finite float32")
    if any(c < 0 or c >= int(ncam_model) for c in ids):
        raise ValueError("voxel_grid: camera index out of range")


def cells(points, bounds, grid):
    """(i int64 [M, 3], q uint32 [M, 3]) of float32 points [M, 3] inside the box: the cell per axis and the position inside it in 1/256."""
    w = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    lo = np.asarray(bounds, dtype=np.float32).reshape(6)[:3]
    g = np.array(grid, dtype=np.float32)
    inv, _ = cell_scale(bounds, grid)
    u = (w - lo) * inv
    fi = np.minimum(np.floor(u), g - F(1.0))
    frac = u - fi
    q = np.clip((frac * F(256.0)).astype(np.int64), 0, 255)
    return fi.astype(np.int64), q.astype(np.uint32)


def accumulate(i, q, rgb, grid):
    """The seven uint32 sums per cell, [gx, gy, gz, 7]: count, sum q (3), sum colour (3; rgb uint8 [M, 3] or None)."""
    gx, gy, gz = grid
    acc = np.zeros((gx * gy * gz, 7), dtype=np.uint32)
    flat = (i[:, 0] * gy + i[:, 1]) * gz + i[:, 2]
    np.add.at(acc[:, 0], flat, np.uint32(1))
    for k in range(3):
        np.add.at(acc[:, 1 + k], flat, q[:, k])
        if rgb is not None:
            np.add.at(acc[:, 4 + k], flat, rgb[:, k].astype(np.uint32))
    return acc.reshape(gx, gy, gz, 7)


def finish(acc, bounds, grid):
    """The eight float32 channels [gx, gy, gz, 8] of the sums."""
    gx, gy, gz = grid
    lo = np.asarray(bounds, dtype=np.float32).reshape(6)[:3]
    _, size = cell_scale(bounds, grid)
    out = np.zeros((gx, gy, gz, CHANNELS), dtype=np.float32)
    occ = acc[..., 0] > 0
    cnt = acc[..., 0][occ].astype(np.float32)
    idx = np.nonzero(occ)
    for k in range(3):
        mean_q = acc[..., 1 + k][occ].astype(np.float32) / cnt
        out[..., k][occ] = lo[k] + (idx[k].astype(np.float32) + (mean_q + F(0.5)) * F(1.0 / 256.0)) * size[k]
        out[..., 3 + k][occ] = (acc[..., 4 + k][occ].astype(np.float32) / cnt) * F(1.0 / 255.0)
    out[..., 6][occ] = cnt
    out[..., 7][occ] = F(1.0)
    return out


def voxel_grid_env(pose, depth, rgb, bounds, max_depth, grid):
    """float32 [gx, gy, gz, 8] of one env: pose [ncam, 16], depth [ncam, H, W], rgb uint8 [ncam, H, W, 3] or None."""
    grid = grid_dims(grid)
    world = pc.deproject(pose, depth)
    cand = pc.candidates(world, depth, bounds, max_depth)
    i, q = cells(world.reshape(-1, 3)[cand], bounds, grid)
    colour = None if rgb is None else np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)[cand]
    return finish(accumulate(i, q, colour, grid), bounds, grid)


def voxel_grid_reference(poses, depth, rgb, bounds, max_depth, grid):
    """The specification of avsim_voxel_grid: poses float32 [N, ncam, 16] (avsim_camera_poses), depth float32 [N, ncam, H, W], rgb uint8
    [N, ncam, H, W, 3] (avsim_render_rgb's env-major layout) or None -> float32 [N, gx, gy, gz, 8]."""
    depth = np.asarray(depth, dtype=np.float32)
    N = depth.shape[0]
    poses = np.asarray(poses, dtype=np.float32).reshape(N, depth.shape[1], pc.POSE_WIDTH)
    return np.stack([voxel_grid_env(poses[n], depth[n], None if rgb is None else rgb[n], bounds, max_depth, grid) for n in range(N)])
