"""The geometric op of av_aloha_amd/imgaug.py (bit 5, the specification of avsim_image_augment) and its plan, against facts that do not depend
on it: numpy's matrix inverse, np.rot90 and slices, a float64 restatement of the nearest rule, scipy's map_coordinates for the bilinear one,
the plan's counts.  No device."""
import numpy as np
import pytest
from scipy import ndimage

from av_aloha_amd import imgaug
from avsim_test_util import bits, noise

A = 32                          # imgaug.AFFINE


def coords64(H, W, M):
    """The source coordinates of the specification's formula in float64, from the float32 matrix."""
    m = np.asarray(M, dtype=np.float32).astype(np.float64)
    xf = (np.arange(W, dtype=np.float64) + 0.5 - W / 2)[None, :]
    yf = (np.arange(H, dtype=np.float64) + 0.5 - H / 2)[:, None]
    return m[0] * xf + m[1] * yf + m[2] + (W / 2 - 0.5), m[3] * xf + m[4] * yf + m[5] + (H / 2 - 0.5)


def test_the_matrix_is_the_inverse_of_the_forward_transform():
    """affine_matrix64 against np.linalg.inv of T . scale . R . SHy . SHx built here in float64: 1000 random parameter sets, angles +-180,
    shears +-30, scale 0.5..2, translations +-50.  Tolerance 1e-12; affine_matrix is its rounding to float32."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for _ in range(1000):
        ang, sx, sy = rng.uniform(-180, 180), rng.uniform(-30, 30), rng.uniform(-30, 30)
        sc, tx, ty = rng.uniform(0.5, 2), rng.uniform(-50, 50), rng.uniform(-50, 50)
        a, bx, by = np.radians(ang), np.radians(sx), np.radians(sy)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        SHx = np.array([[1, -np.tan(bx), 0], [0, 1, 0], [0, 0, 1]])
        SHy = np.array([[1, 0, 0], [-np.tan(by), 1, 0], [0, 0, 1]])
        T = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])
        S = np.diag([sc, sc, 1.0])
        want = np.linalg.inv(T @ S @ R @ SHy @ SHx)[:2].reshape(6)
        got = imgaug.affine_matrix64(ang, tx, ty, sc, sx, sy)
        got32 = imgaug.affine_matrix(ang, tx, ty, sc, sx, sy)
        assert got.dtype == np.float64 and got32.dtype == np.float32 and got.shape == got32.shape == (6,) and np.array_equal(got32, got.astype(np.float32))
        worst = max(worst, np.abs(got - want).max())
    print(f"affine_matrix64 against np.linalg.inv: worst difference {worst:.3g}")
    assert worst <= 1e-12


def test_exact_facts():
    for H, W in ((1, 1), (2, 5), (9, 9), (35, 133)):
        x = imgaug.to_float(noise((H, W, 3), H * W))
        for interp in (0, 1):
            assert np.array_equal(bits(imgaug.affine_reference(x, imgaug.IDENTITY_MATRIX, interp)), bits(x))
            assert np.array_equal(bits(imgaug.affine_reference(x, imgaug.affine_matrix(0.0), interp)), bits(x))
            # a translation larger than the image: all fill
            for t in ((W + 1, 0), (0, -(H + 1)), (-(W + 1), H + 1)):
                assert (imgaug.affine_reference(x, imgaug.affine_matrix(0, *t), interp) == 0).all()
    # quarter turns of a square image, even and odd side
    for n in (8, 9):
        x = imgaug.to_float(noise((n, n, 3), n))
        for angle, k in ((90, 3), (180, 2), (-90, 1)):
            assert np.array_equal(imgaug.affine_reference(x, imgaug.affine_matrix(angle), 0), np.rot90(x, k)), (n, angle)
    # an integer translation: a shifted slice, zero fill
    x = imgaug.to_float(noise((7, 11, 3), 3))
    for tx, ty in ((2, 0), (0, 3), (-4, 1), (3, -2), (-10, -6)):
        want = np.zeros_like(x)
        ys, yd = (slice(0, 7 - ty), slice(ty, 7)) if ty >= 0 else (slice(-ty, 7), slice(0, 7 + ty))
        xs, xd = (slice(0, 11 - tx), slice(tx, 11)) if tx >= 0 else (slice(-tx, 11), slice(0, 11 + tx))
        want[yd, xd] = x[ys, xs]
        for interp in (0, 1):
            assert np.array_equal(bits(imgaug.affine_reference(x, imgaug.affine_matrix(0, tx, ty), interp)), bits(want)), (tx, ty, interp)
    # through the whole reference: bit 5 alone with the identity is mask 0; the fill is normalised
    u = noise((2, 7, 11, 3), 4)
    p = imgaug.pack_params([(1, 2, 1), (0, 0, 0)], [A, A], np.tile(imgaug.IDENTITY, (2, 1)))
    q = imgaug.pack_params([(1, 2, 1), (0, 0, 0)], [0, 0], np.tile(imgaug.IDENTITY, (2, 1)))
    mats = np.tile(imgaug.IDENTITY_MATRIX, (2, 1))
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    assert np.array_equal(bits(imgaug.jitter_affine_reference(u, p, mats, 0, (4, 5), mean, std)), bits(imgaug.jitter_reference(u, q, (4, 5), mean, std)))
    assert np.array_equal(bits(imgaug.jitter_affine_reference(u, q, None, 1, (4, 5), mean, std)), bits(imgaug.jitter_reference(u, q, (4, 5), mean, std)))
    mats[:] = imgaug.affine_matrix(0, 40, 0)
    gone = imgaug.jitter_affine_reference(u, p, mats, 0, (4, 5), mean, std)
    fill = (np.zeros(3, np.float32) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert all((gone[:, c] == fill[c]).all() for c in range(3))


def test_nearest_against_a_float64_restatement():
    """Source coordinates in float64 (coords64), rounded half to even, inside iff 0 <= xi <= W - 1 and 0 <= yi <= H - 1, fill 0.  Pixels whose
    float64 coordinate lies within 1e-3 of a half-integer in x or y are left out (float32's coordinate may round the other way there);
    everything else must be equal, and at most 1 % of the pixels may be left out.  35 x 133, 5 x 67 and 48 x 64 with a random angle, scale
    0.7..1.4 and shear +-10, and 480 x 640 at +-5 degrees with a translation."""
    rng = np.random.default_rng(2)
    cases = []
    for H, W in ((35, 133), (5, 67), (48, 64)):
        for _ in range(50):
            cases.append((H, W, imgaug.affine_matrix(rng.uniform(-180, 180), rng.integers(-W // 4, W // 4 + 1), rng.integers(-H // 4, H // 4 + 1), rng.uniform(0.7, 1.4),
                                                     rng.uniform(-10, 10), rng.uniform(-10, 10))))
    cases += [(480, 640, imgaug.affine_matrix(5.0, 32, -24)), (480, 640, imgaug.affine_matrix(-5.0, -17, 9))]
    total = left_out = 0
    images = {}
    for H, W, M in cases:
        x = images.setdefault((H, W), imgaug.to_float(noise((H, W, 3), H + W)))
        got = imgaug.affine_reference(x, M, 0)
        sx, sy = coords64(H, W, M)
        band = (np.abs(sx - np.floor(sx) - 0.5) < 1e-3) | (np.abs(sy - np.floor(sy) - 0.5) < 1e-3)
        xi, yi = np.rint(sx), np.rint(sy)
        inside = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        want = np.where(inside[..., None], x[np.where(inside, yi, 0).astype(int), np.where(inside, xi, 0).astype(int)], np.float32(0))
        assert np.array_equal(got[~band], want[~band]), (H, W, M)
        total += H * W
        left_out += int(band.sum())
    print(f"nearest: {left_out} of {total} pixels left out ({100 * left_out / total:.2f} %)")
    assert left_out <= 0.01 * total


def test_bilinear_against_map_coordinates():
    """scipy.ndimage.map_coordinates(order=1, mode="grid-constant", cval=0) in float64 at the float64 coordinates of the same formula
    (coords64), against the float32 specification: 20 draws (any angle, scale 0.7..1.4, shear +-10, a translation) for each of 1 x 1, 2 x 5,
    3 x 3, 5 x 67, 35 x 133 and 120 x 160.  The difference is the float32 coordinate's rounding times the image's slope (noise: up to 1 per
    pixel) plus the blend's own roundings.  Measured with this specification: max abs difference 1.705e-5 over the 120 draws; asserted: four
    times that, 6.82e-5."""
    rng = np.random.default_rng(3)
    worst = 0.0
    for H, W in ((1, 1), (2, 5), (3, 3), (5, 67), (35, 133), (120, 160)):
        x = imgaug.to_float(noise((H, W, 3), 7 * H + W))
        for _ in range(20):
            M = imgaug.affine_matrix(rng.uniform(-180, 180), rng.integers(-(W // 4), W // 4 + 1), rng.integers(-(H // 4), H // 4 + 1), rng.uniform(0.7, 1.4),
                                     rng.uniform(-10, 10), rng.uniform(-10, 10))
            got = imgaug.affine_reference(x, M, 1)
            sx, sy = coords64(H, W, M)
            want = np.stack([ndimage.map_coordinates(x[..., c].astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0) for c in range(3)], axis=-1)
            assert got.dtype == np.float32 and not np.isnan(got).any()
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"bilinear against map_coordinates: max abs difference {worst:.4g}")
    assert worst <= 4 * 1.705e-5


def test_plan_with_and_without_affine():
    kw = dict(seed=3, epoch=1, batch=2, camera_index=1)
    a = imgaug.augment_plan(300, None, **kw)
    for cfg in (None, True, {"affine": {"weight": 0}}, {"affine": {"weight": 0.0, "degrees": 30}}):
        m, f, M, d = imgaug.augment_plan_affine(300, cfg, size=(48, 64), **kw)
        assert np.array_equal(m, a[0]) and np.array_equal(bits(f), bits(a[1]))
        assert M.dtype == np.float32 and (M == imgaug.IDENTITY_MATRIX).all() and (d == imgaug.IDENTITY_DRAWN).all()
    H, W = 480, 640
    m, f, M, d = imgaug.augment_plan_affine(2000, imgaug.LEROBOT_CFG, size=(H, W), **kw)
    assert m.dtype == np.int32 and f.dtype == np.float32 and M.dtype == np.float32 and d.dtype == np.float64 and M.shape == d.shape == (2000, 6)
    assert (sum((m >> k) & 1 for k in range(6)) == 3).all()
    for k in range(6):
        share = (m >> k & 1).mean()
        print(f"op {k}: chosen for {share:.3f} of 2000 images")
        assert 0.44 <= share <= 0.56            # 50 % expected, sigma about 1.1 %
    on = (m & A).astype(bool)
    assert (M[~on] == imgaug.IDENTITY_MATRIX).all() and (d[~on] == imgaug.IDENTITY_DRAWN).all()
    assert ((d[on, 0] >= -5) & (d[on, 0] <= 5)).all() and np.unique(d[on, 0]).size > 900
    assert (d[on, 1] == np.rint(d[on, 1])).all() and (np.abs(d[on, 1]) <= 0.05 * W).all() and np.unique(d[on, 1]).size > 40
    assert (d[on, 2] == np.rint(d[on, 2])).all() and (np.abs(d[on, 2]) <= 0.05 * H).all() and np.unique(d[on, 2]).size > 30
    assert (d[on, 3] == 1).all() and (d[on, 4:] == 0).all()
    for i in np.nonzero(on)[0][:50]:
        assert np.array_equal(bits(M[i]), bits(imgaug.affine_matrix(*d[i])))
    for k, name in enumerate(imgaug.OPS):
        lo, hi = (np.float32(v) for v in imgaug.DEFAULT_CFG[name]["min_max"])
        sel = (m >> k & 1).astype(bool)
        assert ((f[sel, k] >= lo) & (f[sel, k] <= hi)).all() and (f[~sel, k] == imgaug.IDENTITY[k]).all()
    imgaug.check_jitter_affine((1, H, W), imgaug.pack_params(np.zeros((2000, 3)), m, f), M, 0, (H, W), src_index=np.zeros(2000, int))
    # scale and shears are drawn when their ranges are given, inside them
    cfg = dict(imgaug.DEFAULT_CFG, max_num_transforms=6, affine={"degrees": 30, "translate": None, "scale": (0.7, 1.4), "shear": (-10, 10, -3, 3), "interpolation": "bilinear"})
    m, f, M, d = imgaug.augment_plan_affine(200, cfg, size=(48, 64), **kw)
    assert (m == 63).all() and (np.abs(d[:, 0]) <= 30).all() and (d[:, 1:3] == 0).all() and ((d[:, 3] >= 0.7) & (d[:, 3] <= 1.4)).all()
    assert (np.abs(d[:, 4]) <= 10).all() and (np.abs(d[:, 5]) <= 3).all() and np.unique(d[:, 5]).size > 150
    assert imgaug.interp_of(imgaug.make_cfg(cfg)) == 1 and imgaug.interp_of(imgaug.make_cfg(imgaug.LEROBOT_CFG)) == 0
    # DEFAULT_CFG has no affine, and make_cfg of it returns none
    assert "affine" not in imgaug.DEFAULT_CFG and "affine" not in imgaug.make_cfg(True) and not imgaug.has_affine(imgaug.make_cfg(None))
    for bad in ({"affine": 1}, {"affine": {"weight": -1}}, {"affine": {"angle": 3}}, {"affine": {"translate": (0.1, 2)}}, {"affine": {"scale": (0, 1)}},
                {"affine": {"shear": (1, 2, 3)}}, {"affine": {"interpolation": "bicubic"}}, {"affine": {"degrees": (5, -5)}}):
        with pytest.raises(ValueError):
            imgaug.make_cfg(bad)
    with pytest.raises(ValueError):
        imgaug.augment_plan_affine(4, imgaug.LEROBOT_CFG)              # no size


def test_check_jitter_affine_refuses():
    ok = dict(src_shape=(3, 7, 9), boxes=[(1, 1, 0), (4, 3, 1)], masks=[63, 32], factors=[[1, 1, 1, 0, 1]] * 2, matrix=[[1, 0, 0, 0, 1, 0]] * 2, interp=0,
              out_hw=(4, 5), mean=None, std=None, src_index=None)

    def check(**kw):
        a = dict(ok, **kw)
        p = imgaug.pack_params(np.asarray(a["boxes"], dtype=np.int32).reshape(-1, 3), a["masks"], np.asarray(a["factors"], dtype=np.float32).reshape(-1, 5))
        imgaug.check_jitter_affine(a["src_shape"], p, a["matrix"], a["interp"], a["out_hw"], a["mean"], a["std"], a["src_index"])

    nan, inf, big = float("nan"), float("inf"), float(2 ** 20)
    check()
    check(interp=1)
    check(masks=[31, 0], matrix=None)                                                   # no bit 5: no matrices needed
    check(masks=[31, 32], matrix=[[nan, inf, -inf, 1e30, nan, nan], [1, 0, 0, 0, 1, 0]])    # entries of unset bits are not read
    check(matrix=[[big, -big, big, -big, big, -big], [1, 0, 0, 0, 1, 0]])               # the limit itself
    check(masks=[32, 32], factors=[[nan, inf, -1, 9, 99]] * 2)                          # factors of unset bits are not looked at
    refused = [dict(masks=[64, 0]), dict(masks=[0, -1]), dict(masks=[0, 95]), dict(interp=2), dict(interp=-1), dict(matrix=None), dict(masks=[0, 32], matrix=None)]
    for k in range(6):
        for v in (nan, inf, -inf, big * 1.001, -big * 1.001):
            m = [1.0, 0, 0, 0, 1, 0]
            m[k] = v
            refused.append(dict(matrix=[[1, 0, 0, 0, 1, 0], m]))
    # check_jitter's own conditions hold with bit 5 set
    refused += [dict(boxes=[(5, 1, 0), (0, 0, 0)]), dict(boxes=[(0, 0, 2), (0, 0, 0)]), dict(src_index=[3, 0]), dict(out_hw=(8, 5)), dict(src_shape=(3, 0, 9)),
                dict(factors=[[1, 1, 1, 0.6, 1]] * 2), dict(factors=[[17, 1, 1, 0, 1]] * 2), dict(mean=[0.5] * 3, std=[0.2, 0, 0.2]), dict(mean=[0.5] * 3)]
    for kw in refused:
        with pytest.raises(ValueError):
            check(**kw)
    u = noise((3, 7, 9, 3), 5)
    with pytest.raises(ValueError):
        imgaug.jitter_affine_reference(u, imgaug.pack_params([(0, 0, 0)], [32], [imgaug.IDENTITY]), [[nan, 0, 0, 0, 1, 0]], 0, (4, 5))
    with pytest.raises(ValueError):
        imgaug.affine_reference(imgaug.to_float(u[0]), imgaug.IDENTITY_MATRIX, 2)
    # the existing check keeps refusing bit 5
    with pytest.raises(ValueError):
        imgaug.check_jitter((3, 7, 9), imgaug.pack_params([(0, 0, 0)], [32], [imgaug.IDENTITY]), (4, 5))
