"""The specification of avsim_virtual_views (av_aloha_amd/virtviews.py) on its own, no GPU: where a point lands in each of the six views,
occlusion, ties, footprints, the box's faces, dropped pixels, the checks, and the whole of it against an independent float64 brute force.

The small cases use cameras of 1 x 1 pixels with an identity rotation: the one ray is the camera's -z, so camera s at (x, y, 1) with depth d
is the world point (x, y, 1 - d), and its flat slot is s."""
import numpy as np
import pytest

from av_aloha_amd import pointcloud as pc
from av_aloha_amd import virtviews as vv

UNIT = np.array([0, 0, 0, 1, 1, 1], dtype=np.float32)
ALL = ("+x", "-x", "+y", "-y", "+z", "-z")
FAR = pc.FAR_PLANE


def points_as_cameras(points):
    """(pose [n, 16], depth [n, 1, 1]) whose deprojection is the given world points, one camera of one pixel each."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pose = np.zeros((len(p), 16), dtype=np.float32)
    pose[:, 0], pose[:, 1], pose[:, 2] = p[:, 0], p[:, 1], 1.0
    pose[:, 3] = pose[:, 7] = pose[:, 11] = 1.0
    pose[:, 12] = 0.5
    return pose, (1.0 - p[:, 2]).astype(np.float32).reshape(-1, 1, 1)


def render(points, views=ALL, size=(4, 8), radius=0, bounds=UNIT, rgb=None, max_depth=FAR):
    pose, depth = points_as_cameras(points)
    return vv.virtual_views_env(pose, depth, rgb, bounds, max_depth, views, size, radius)


def where(index, v):
    """(row, column) of the hit pixels of view v."""
    return [tuple(int(x) for x in rc) for rc in np.argwhere(index[v] >= 0)]


def test_view_names_and_codes():
    assert vv.VIEW_NAMES == ALL and vv.view_codes(ALL) == (0, 1, 2, 3, 4, 5)
    assert vv.view_codes(["+z", 0, "-x", "+z"]) == (4, 0, 1, 4) and vv.view_codes("+y") == (2,) and vv.view_codes(np.array([5, 3])) == (5, 3)
    with pytest.raises(ValueError):
        vv.view_codes(["up"])
    assert vv.view_size(7) == (7, 7) and vv.view_size((3, 9)) == (3, 9)
    with pytest.raises(ValueError):
        vv.view_size((1, 2, 3))


def test_one_point_in_each_of_the_six_views():
    """(0.3, 0.6, 0.2) in the unit box, views of 4 x 8: x is column 2 of 8, y column 4 of 8 and row 2 of 4, z row 0 of 4, counted ascending."""
    out, index = render([(0.3, 0.6, 0.2)])
    assert out.shape == (6, 4, 8, 8) and out.dtype == np.float32 and index.shape == (6, 4, 8) and index.dtype == np.int32
    assert [where(index, v) for v in range(6)] == [[(3, 4)], [(3, 3)], [(3, 5)], [(3, 2)], [(1, 2)], [(2, 2)]]
    want_dist = [0.7, 0.3, 0.4, 0.6, 0.8, 0.2]
    for v, (r, c) in enumerate([(3, 4), (3, 3), (3, 5), (3, 2), (1, 2), (2, 2)]):
        px = out[v, r, c]
        assert index[v, r, c] == 0 and px[7] == 1.0 and abs(px[3] - want_dist[v]) < 1e-6 and np.allclose(px[4:7], (0.3, 0.6, 0.2), atol=1e-6) and not px[:3].any()
        assert np.count_nonzero(out[v]) == 5          # dist, the point, the flag: every other pixel is zeros


def test_a_moved_point_moves_the_way_the_table_says():
    base = np.array([0.3, 0.6, 0.2])
    at = lambda p: [where(render([p])[1], v)[0] for v in range(6)]
    a, y, x, z = at(base), at(base + (0, 0.25, 0)), at(base + (0.25, 0, 0)), at(base + (0, 0, 0.3))
    # toward hi-y: right in +x, left in -x, up in +z, down in -z, nothing in +-y
    assert y[0][1] > a[0][1] and y[1][1] < a[1][1] and y[4][0] < a[4][0] and y[5][0] > a[5][0] and y[2] == a[2] and y[3] == a[3]
    assert y[0][0] == a[0][0] and y[1][0] == a[1][0] and y[4][1] == a[4][1] and y[5][1] == a[5][1]
    # toward hi-x: left in +y, right in -y, +z and -z, nothing in +-x
    assert x[2][1] < a[2][1] and x[3][1] > a[3][1] and x[4][1] > a[4][1] and x[5][1] > a[5][1] and x[0] == a[0] and x[1] == a[1]
    # toward hi-z: up in the four side views, nothing from above and below
    assert all(z[v][0] < a[v][0] and z[v][1] == a[v][1] for v in range(4)) and z[4] == a[4] and z[5] == a[5]


def test_occlusion():
    """Two points over the same pixel: +z shows the upper one, -z the lower one; from the side both are seen."""
    rgb = np.array([[[[255, 0, 0]]], [[[0, 51, 255]]]], dtype=np.uint8)
    out, index = render([(0.5, 0.5, 0.7), (0.5, 0.5, 0.4)], rgb=rgb)
    top, bottom = where(index, 4), where(index, 5)
    assert len(top) == 1 and len(bottom) == 1
    assert index[4][top[0]] == 0 and index[5][bottom[0]] == 1
    assert out[4][top[0]][:3].tolist() == [1.0, 0.0, 0.0] and out[5][bottom[0]][:3].tolist() == [0.0, float(np.float32(51) * np.float32(1 / 255)), 1.0]
    assert abs(out[4][top[0]][3] - 0.3) < 1e-6 and abs(out[5][bottom[0]][3] - 0.4) < 1e-6
    assert len(where(index, 0)) == 2
    # the order of the cameras does not decide it
    _, swapped = render([(0.5, 0.5, 0.4), (0.5, 0.5, 0.7)])
    assert swapped[4][top[0]] == 1 and swapped[5][bottom[0]] == 0


def test_a_tie_goes_to_the_lower_slot():
    _, index = render([(0.2, 0.2, 0.5), (0.5, 0.5, 0.3), (0.5, 0.5, 0.3), (0.5, 0.5, 0.3)])
    for v in range(6):
        assert sorted(set(index[v][index[v] >= 0].tolist())) == [0, 1], v
    # and with a footprint: where the footprints of equal dists overlap the lower slot wins, elsewhere each is seen
    _, index = render([(0.30, 0.5, 0.5), (0.45, 0.5, 0.5)], views=["-y"], size=(8, 8), radius=1)
    assert index[0, 2:5].tolist() == [[-1, 0, 0, 0, 1, -1, -1, -1]] * 3 and (index[0, :2] == -1).all() and (index[0, 5:] == -1).all()          # (z = 0.5 is row 3 of 8)


@pytest.mark.parametrize("r", [0, 1, 2, 4])
def test_footprint(r):
    n = 2 * r + 1
    _, index = render([(0.5, 0.5, 0.5)], size=(16, 16), radius=r)
    for v in range(6):
        rows, cols = np.nonzero(index[v] >= 0)
        assert len(rows) == n * n and rows.max() - rows.min() == 2 * r and cols.max() - cols.min() == 2 * r
    # in a corner it is clipped: (r + 1)^2 pixels stay
    _, index = render([(0.01, 0.01, 0.01)], size=(16, 16), radius=r)
    for v in range(6):
        assert (index[v] >= 0).sum() == (r + 1) ** 2
    # a footprint larger than the image covers it
    _, index = render([(0.5, 0.5, 0.5)], size=(3, 3), radius=4)
    assert (index == 0).all()


def test_a_point_on_hi_goes_to_the_last_pixel():
    out, index = render([(1.0, 1.0, 1.0), (0.0, 0.0, 0.0)])
    assert [where(index, v) for v in range(6)] == [[(0, 7), (3, 0)], [(0, 0), (3, 7)], [(0, 0), (3, 7)], [(0, 7), (3, 0)], [(0, 7), (3, 0)], [(0, 0), (3, 7)]]
    # on the face the dist is +0, and the far face's is the extent
    assert out[0, 0, 7, 3].view(np.int32) == 0 and out[0, 3, 0, 3] == 1.0 and out[5, 0, 0, 3].view(np.int32) == 0 and index[5, 0, 0] == 1


def test_nan_infinite_and_far_depths_drop_the_pixel():
    pose, depth = points_as_cameras([(0.5, 0.5, 0.5)] * 4 + [(0.2, 0.2, 0.2)])
    depth[0], depth[1], depth[2] = np.nan, np.inf, -np.inf
    _, index = vv.virtual_views_env(pose, depth, None, UNIT, FAR, ALL, (4, 8), 1)
    assert set(index[index >= 0].tolist()) == {3, 4}
    _, index = vv.virtual_views_env(pose, depth, None, UNIT, 0.6, ALL, (4, 8), 1)          # d < max_depth: the point at depth 0.8 goes too
    assert set(index[index >= 0].tolist()) == {3}


def test_an_env_without_candidates_is_zeros():
    out, index = render([(0.5, 0.5, 1.5), (2.0, 0.5, 0.5)], radius=2, rgb=np.full((2, 1, 1, 3), 200, dtype=np.uint8))
    assert (out.view(np.int32) == 0).all() and (index == -1).all()


def test_check_refuses_what_the_header_refuses():
    good = dict(ncam_model=6, cam_ids=[0, 3], height=24, width=32, bounds=[-1, -1, 0, 1, 1, 2], max_depth=30.0, views=[4, 0, 1, 2, 3], size=(220, 220), radius=1)
    vv.check_virtual_views(**good)
    vv.check_virtual_views(**{**good, "views": ["+z"] * 6, "size": (1024, 1), "radius": 4, "cam_ids": list(range(6)) * 2 + [0, 1, 2, 3]})
    vv.check_virtual_views(**{**good, "radius": 0, "size": 1})
    nan, inf = float("nan"), float("inf")
    b = lambda k, v: [v if i == k else x for i, x in enumerate(good["bounds"])]
    bad = [dict(cam_ids=[]), dict(cam_ids=[0] * 17), dict(cam_ids=[0, 6]), dict(cam_ids=[-1]), dict(height=0), dict(width=65536), dict(height=4097, width=2048),
           dict(views=[]), dict(views=[0] * 7), dict(views=[6]), dict(views=[0, -1]), dict(views=["front"]), dict(size=0), dict(size=(1025, 4)), dict(size=(4, -1)),
           dict(size=(1, 2, 3)), dict(radius=-1), dict(radius=5), dict(radius=1.5), dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=inf), dict(max_depth=nan),
           dict(bounds=b(1, nan)), dict(bounds=b(4, inf)), dict(bounds=b(2, 60.0)), dict(bounds=b(0, 1.0)), dict(bounds=good["bounds"][:5]),
           dict(bounds=[0, 0, 0, 1, 1, 1e-37], size=1024), dict(bounds=[-3e38, 0, 0, 3e38, 1, 1])]
    for kw in bad:
        with pytest.raises(ValueError):
            vv.check_virtual_views(**{**good, **kw})


def test_reference_stacks_envs():
    rng = np.random.default_rng(3)
    poses = np.stack([two_cameras(0.0), two_cameras(0.2), two_cameras(-0.3)])
    depth = rng.uniform(0.3, 1.5, (3, 2, 6, 8)).astype(np.float32)
    rgb = rng.integers(0, 256, (3, 2, 6, 8, 3), dtype=np.uint8)
    out, index = vv.virtual_views_reference(poses, depth, rgb, BOX, FAR, ["+z", "-y"], (5, 7), 1)
    assert out.shape == (3, 2, 5, 7, 8) and out.dtype == np.float32 and index.shape == (3, 2, 5, 7) and index.dtype == np.int32
    for n in range(3):
        o, i = vv.virtual_views_env(poses[n], depth[n], rgb[n], BOX, FAR, [4, 3], (5, 7), 1)
        assert o.tobytes() == out[n].tobytes() and i.tobytes() == index[n].tobytes()
    assert (index >= 0).any(1).any(1).any(1).all() and not np.array_equal(index[0], index[1])
    no_colour, i2 = vv.virtual_views_reference(poses, depth, None, BOX, FAR, ["+z", "-y"], (5, 7), 1)
    assert np.array_equal(i2, index) and not no_colour[..., :3].any() and np.array_equal(no_colour[..., 3:], out[..., 3:])


# ---- against an independent float64 brute force ----------------------------------------------------------------------------------------

BOX = np.array([-1.0, -1.0, -0.6, 1.0, 1.0, 1.0], dtype=np.float32)
SEED = 5


def look_at(eye, target, tan):
    """A pose record of a camera at `eye` that looks along its -z at `target`, x to the right, y up."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    rec = np.zeros(16, dtype=np.float32)
    rec[:3], rec[3:12], rec[12] = eye, np.stack([right, up, back], axis=1).reshape(-1), tan
    return rec


def two_cameras(shift):
    return np.stack([look_at((1.1 + shift, 0.3, 0.9), (0, 0, 0.1), 0.45), look_at((-0.7, -1.0 + shift, 0.8), (0.1, 0, 0), 0.6)])


def brute_force(pose, depth, cand, bounds, code, size, radius):
    """float64, per virtual pixel a loop over all candidates -> (the winner's slot or -1 [VH, VW], the pixels excepted from the comparison
    [VH, VW]: one of the candidates that may cover it lies within 1e-4 of a pixel border in either image coordinate, or two candidates that
    cover it have dists closer than 1e-6)."""
    vh, vw = size
    pose, b = pose.astype(np.float64), bounds.astype(np.float64)
    ncam, H, W = depth.shape
    pts = np.empty((ncam, H, W, 3))
    for s in range(ncam):
        p, R, t = pose[s, :3], pose[s, 3:12].reshape(3, 3), pose[s, 12]
        scale = 2.0 * t / H
        x, y = ((np.arange(W) + 0.5) - 0.5 * W) * scale, -(((np.arange(H) + 0.5) - 0.5 * H) * scale)
        d = depth[s].astype(np.float64)
        cam = np.stack([x[None, :] * d, y[:, None] * d, -d], axis=-1)
        pts[s] = p + cam @ R.T
    w = pts.reshape(-1, 3)[cand]
    da, from_hi, ca, cdesc, ra, rdesc = [(0, 1, 1, 0, 2, 1), (0, 0, 1, 1, 2, 1), (1, 1, 0, 1, 2, 1), (1, 0, 0, 0, 2, 1), (2, 1, 0, 0, 1, 1), (2, 0, 0, 0, 1, 0)][code]
    dist = b[3 + da] - w[:, da] if from_hi else w[:, da] - b[da]
    uc, ur = (w[:, ca] - b[ca]) / (b[3 + ca] - b[ca]) * vw, (w[:, ra] - b[ra]) / (b[3 + ra] - b[ra]) * vh
    col, row = np.minimum(np.floor(uc), vw - 1).astype(int), np.minimum(np.floor(ur), vh - 1).astype(int)
    col, row = (vw - 1 - col if cdesc else col), (vh - 1 - row if rdesc else row)
    shaky = (np.abs(uc - np.round(uc)) < 1e-4) | (np.abs(ur - np.round(ur)) < 1e-4)
    winner, excepted = np.full((vh, vw), -1, dtype=np.int64), np.zeros((vh, vw), dtype=bool)
    for r in range(vh):
        for c in range(vw):
            near = (np.abs(row - r) <= radius + 1) & (np.abs(col - c) <= radius + 1)          # (a shaky candidate may be one pixel off)
            cover = (np.abs(row - r) <= radius) & (np.abs(col - c) <= radius)
            excepted[r, c] = (shaky & near).any()
            k = np.nonzero(cover)[0]
            if len(k):
                order = np.lexsort((cand[k], dist[k]))
                winner[r, c] = cand[k[order[0]]]
                ds = np.sort(dist[k])
                excepted[r, c] |= len(k) > 1 and (np.diff(ds) < 1e-6).any()
    return winner, excepted


@pytest.mark.parametrize("radius", [0, 1])
def test_against_a_float64_brute_force(radius):
    """Noise depth in [0.3, 1.5] on 2 cameras of 24 x 32, all six views at 16 x 16: the winner's slot is the brute force's at every virtual
    pixel but the excepted ones, and those are at most 2 % of the pixels (a condition: the seed was picked so that the specification alone
    meets it)."""
    rng = np.random.default_rng(SEED)
    pose = two_cameras(0.0)
    depth = rng.uniform(0.3, 1.5, (2, 24, 32)).astype(np.float32)
    cand = pc.candidates(pc.deproject(pose, depth), depth, BOX, FAR)
    assert 400 < len(cand) < 2 * 24 * 32
    _, index = vv.virtual_views_env(pose, depth, None, BOX, FAR, ALL, (16, 16), radius)
    excepted_total = 0
    for code in range(6):
        winner, excepted = brute_force(pose, depth, cand, BOX, code, (16, 16), radius)
        differs = (winner != index[code]) & ~excepted
        assert not differs.any(), f"view {ALL[code]}: the winner differs at {np.argwhere(differs)[:4].tolist()}"
        assert (winner >= 0).sum() > 20
        excepted_total += int(excepted.sum())
    print(f"radius {radius}: {excepted_total} of {6 * 256} virtual pixels excepted")
    assert excepted_total <= 0.02 * 6 * 256
