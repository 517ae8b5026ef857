"""The specification of avsim_point_cloud (av_aloha_amd/pointcloud.py) on the host: deprojection, crop, cap and farthest point sampling
against scalar Python, the geometry of the pixel rays, ties, degenerate candidate counts and the refusals.  No device here: the device is
compared with this specification bit for bit in tests/test_gpu_pointcloud.py."""
import numpy as np
import pytest

from av_aloha_amd import pointcloud as pc

F = np.float32
T45 = F(np.tan(np.deg2rad(45.0) / 2))


def ident_pose(t=T45, pos=(0, 0, 0)):
    p = np.zeros(16, dtype=np.float32)
    p[:3] = pos
    p[3:12] = np.eye(3, dtype=np.float32).reshape(-1)
    p[12] = t
    return p[None]


WIDE = (-100, -100, -100, 100, 100, 100)


def fps_scalar(w, P):
    """The rule of the module docstring, one candidate at a time, with no early exit."""
    M = len(w)
    mind = [F(np.inf)] * M
    sel = [0]
    for _ in range(1, P):
        s = sel[-1]
        best, at = F(-1), -1
        for k in range(M):
            dx, dy, dz = F(w[k][0] - w[s][0]), F(w[k][1] - w[s][1]), F(w[k][2] - w[s][2])
            d = F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
            mind[k] = min(mind[k], d)
            if mind[k] > best:
                best, at = mind[k], k
        sel.append(at)
    return np.array(sel)


def test_fps_equals_a_scalar_loop():
    rng = np.random.default_rng(0)
    for M, P in ((1, 3), (7, 7), (50, 20), (33, 40)):
        w = rng.uniform(-1, 1, (M, 3)).astype(np.float32)
        assert np.array_equal(pc.fps(w, P), fps_scalar(w, P)), (M, P)
    w = np.repeat(rng.uniform(-1, 1, (4, 3)).astype(np.float32), 3, 0)      # duplicates: the distances reach 0 before P selections
    assert np.array_equal(pc.fps(w, 10), fps_scalar(w, 10))


def test_fronto_parallel_plane_under_the_identity_pose():
    H, W = 6, 8
    d = np.full((1, H, W), 0.75, dtype=np.float32)
    w = pc.deproject(ident_pose(), d)
    assert w.shape == (1, H, W, 3) and w.dtype == np.float32
    assert np.array_equal(w[0, :, :, 2], -d[0])
    x, y = pc.pixel_rays(T45, H, W)
    assert np.array_equal(w[0, :, :, 0], np.broadcast_to(x[None, :] * F(0.75), (H, W))) and np.array_equal(w[0, :, :, 1], np.broadcast_to(y[:, None] * F(0.75), (H, W)))
    assert x[0] < 0 < x[-1] and y[0] > 0 > y[-1]            # column 0 is left, row 0 is top (the camera's +y is up)
    assert np.isclose(-y[-1] + (y[0] - y[1]) / 2, T45)       # the image's lower edge is at tan(fovy / 2)


def test_projection_of_a_deprojected_point_is_the_pixel_centre():
    rng = np.random.default_rng(1)
    H, W = 9, 13
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0.0]])
    pose = ident_pose(pos=(0.3, -0.2, 0.9))
    pose[0, 3:12] = R.reshape(-1).astype(np.float32)
    d = rng.uniform(0.3, 1.5, (1, H, W)).astype(np.float32)
    w = pc.deproject(pose, d).astype(np.float64)
    cam = (w - pose[0, :3].astype(np.float64)) @ pose[0, 3:12].reshape(3, 3).astype(np.float64)        # R^T (w - p), per point
    scale = 2.0 * float(T45) / H
    col = cam[..., 0] / -cam[..., 2] / scale + 0.5 * W
    row = -cam[..., 1] / -cam[..., 2] / scale + 0.5 * H
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    assert np.abs(col[0] - (cc + 0.5)).max() < 1e-4 and np.abs(row[0] - (rr + 0.5)).max() < 1e-4
    assert np.abs(-cam[0, :, :, 2] - d[0]).max() < 1e-6


def test_exact_ties_select_the_lowest_position():
    # the corners of a square, then its centre: from corner 0 the opposite corner is farthest; then the two others tie exactly
    w = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 0]], dtype=np.float32)
    assert pc.fps(w, 5).tolist() == [0, 3, 1, 2, 4]
    # a constant depth under the identity pose: a symmetric grid of points
    d = np.full((1, 4, 4), 1.0, dtype=np.float32)
    xyz, index, count = pc.point_cloud_env(ident_pose(), d, WIDE, 10.0, 4)
    assert index.tolist() == [0, 15, 3, 12] and count.tolist() == [16, 4]


def test_fewer_candidates_than_points_repeat_candidate_zero():
    d = np.full((1, 2, 3), 30.0, dtype=np.float32)
    d[0, 0, 1], d[0, 1, 0], d[0, 1, 2] = 0.5, 0.6, 0.7
    xyz, index, count = pc.point_cloud_env(ident_pose(), d, WIDE, 30.0, 6)
    assert count.tolist() == [3, 3]
    assert sorted(index[:3].tolist()) == [1, 3, 5] and index[0] == 1 and index[3:].tolist() == [1, 1, 1]
    assert np.array_equal(xyz[3:], np.repeat(xyz[:1], 3, 0))


def test_no_candidate_gives_zeros_and_minus_one():
    d = np.full((2, 3, 3), 30.0, dtype=np.float32)
    xyz, index, count = pc.point_cloud_reference(np.stack([np.repeat(ident_pose(), 2, 0)]), d[None], WIDE, 30.0, 5)
    assert xyz.shape == (1, 5, 3) and not xyz.any() and (index == -1).all() and count.tolist() == [[0, 0]]
    assert xyz.dtype == np.float32 and index.dtype == np.int32 and count.dtype == np.int32


def test_cap_positions_match_the_integer_formula():
    C = pc.MAX_CANDIDATES
    for M in (C + 1, 3 * C // 2):
        pos = pc.cap_positions(M)
        assert len(pos) == C and pos.tolist() == [(i * M) // C for i in range(C)]
        assert pos[0] == 0 and np.all(np.diff(pos) >= 1) and pos[-1] < M
    assert pc.cap_positions(C + 1)[-1] == C - 1 and pc.cap_positions(C + 1)[C // 2:C // 2 + 2].tolist() == [C // 2, C // 2 + 1]
    assert pc.cap_positions(C).tolist() == list(range(C)) and pc.cap_positions(5).tolist() == [0, 1, 2, 3, 4]
    # through the whole specification, with a small cap
    d = np.full((1, 5, 6), 1.0, dtype=np.float32)
    _, index, count = pc.point_cloud_env(ident_pose(), d, WIDE, 10.0, 30, max_candidates=20)
    assert count.tolist() == [30, 20] and set(index.tolist()) == {(i * 30) // 20 for i in range(20)}


def test_bounds_are_inclusive_and_a_nan_depth_drops_the_pixel():
    d = np.array([[[0.5, 1.0, 2.0, np.nan, 1.0]]], dtype=np.float32)
    pose = ident_pose()
    w = pc.deproject(pose, d)
    # z = -d: the box [-1, -0.5] keeps 0.5 and 1.0 exactly on its faces, drops 2.0 and the NaN
    b = (-100, -100, -1.0, 100, 100, -0.5)
    assert pc.candidates(w, d, b, 10.0).tolist() == [0, 1, 4]
    # x bounds on the points themselves: with s the ray spacing the columns' rays are -2 s, -s, 0, s, 2 s, so pixels 0 and 1 share x = -s
    # (-2 s x 0.5, -s x 1.0) exactly on the lower face, pixel 2 lies at 0 on the upper one and pixel 4 at 2 s outside
    bx = (float(w[0, 0, 1, 0]), -100, -100, float(w[0, 0, 2, 0]), 100, 100)
    assert w[0, 0, 0, 0] == w[0, 0, 1, 0] < 0 and w[0, 0, 2, 0] == 0
    assert pc.candidates(w, d, bx, 10.0).tolist() == [0, 1, 2]
    assert pc.candidates(w, d, WIDE, 1.0).tolist() == [0]                        # d < max_depth is strict
    dn = d.copy()
    dn[0, 0, 0] = np.inf
    assert pc.candidates(pc.deproject(pose, dn), dn, WIDE, 10.0).tolist() == [1, 2, 4]


@pytest.mark.parametrize("kw", [
    {"npoints": 0}, {"npoints": 4097}, {"height": 0}, {"width": 65536}, {"cam_ids": []}, {"cam_ids": list(range(17)), "ncam_model": 32},
    {"cam_ids": [0] * 16, "height": 1025, "width": 1024}, {"bounds": (0, 0, 0, 1, np.inf, 1)}, {"bounds": (0, 0, 0, 1, np.nan, 1)},
    {"bounds": (0, 2, 0, 1, 1, 1)}, {"max_depth": 0.0}, {"max_depth": -1.0}, {"max_depth": np.inf}, {"max_depth": np.nan},
    {"cam_ids": [6]}, {"cam_ids": [-1]}, {"bounds": (0, 0, 0, 1, 1)},
])
def test_check_point_cloud_refuses(kw):
    args = {"ncam_model": 6, "cam_ids": [0, 1], "height": 24, "width": 32, "bounds": (0, 0, 0, 1, 1, 1), "max_depth": 30.0, "npoints": 16}
    pc.check_point_cloud(**args)
    pc.check_point_cloud(**{**args, "npoints": 4096, "height": 65535, "width": 1, "bounds": (0, 0, 0, 0, 0, 0)})
    with pytest.raises(ValueError):
        pc.check_point_cloud(**{**args, **kw})
