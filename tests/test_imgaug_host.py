"""av_aloha_amd/imgaug.py, the specification of avsim_image_jitter and the random plan, against facts that do not depend on it: identities of
the blend, imgprep's normalisation table, colorsys, float64 means, the 1/13 and 5/13 of the blur, the plan's counts.  No device."""
import colorsys

import numpy as np
import pytest

from av_aloha_amd import dataset, imgaug, imgprep
from avsim_test_util import bits, noise

B, C, S, Hh, SH = imgaug.BRIGHTNESS, imgaug.CONTRAST, imgaug.SATURATION, imgaug.HUE, imgaug.SHARPNESS


def params(boxes, masks, factors):
    return imgaug.pack_params(boxes, masks, np.asarray(factors, dtype=np.float32).reshape(-1, 5))


def all_values():
    """u8 [1, 16, 16, 3]: all 256 values in every channel, in three different orders."""
    v = np.arange(256, dtype=np.uint8)
    return np.stack([v, v[::-1], np.roll(v, 77)], axis=-1).reshape(1, 16, 16, 3)


def test_factor_one_returns_the_input_floats():
    u = noise((1, 9, 11, 3), 1)
    want = np.transpose(u[0].astype(np.float32) / np.float32(255), (2, 0, 1))
    for mask in (B, C, S, SH, B | C | S | SH):
        got = imgaug.jitter_reference(u, params([(0, 0, 0)], [mask], [1, 1, 1, 0, 1]), (9, 11))
        assert got.dtype == np.float32 and np.array_equal(bits(got[0]), bits(want)), mask


def test_mask_zero_equals_the_normalisation_table():
    u = all_values()
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    boxes = [(0, 0, 0), (3, 2, 1)]
    got = imgaug.jitter_reference(u, params(boxes, [0, 0], [[7, 7, 7, 7, 7]] * 2), (12, 13), mean, std, [0, 0])
    want = imgprep.prep_reference(u, imgprep.normalise_lut(mean, std), None, boxes, (12, 13), [0, 0])
    assert np.array_equal(bits(got), bits(want))
    full = imgaug.jitter_reference(u, params([(0, 0, 0)], [0], [0] * 5), (16, 16), mean, std)
    assert np.array_equal(bits(full), bits(imgprep.prep_reference(u, imgprep.normalise_lut(mean, std), None, [(0, 0, 0)], (16, 16))))
    plain = imgaug.jitter_reference(u, params([(0, 0, 0)], [0], [0] * 5), (16, 16))
    assert np.array_equal(bits(plain), bits(imgprep.prep_reference(u, imgprep.identity_lut(), None, [(0, 0, 0)], (16, 16))))


def test_factor_zero():
    u = noise((1, 13, 17, 3), 2)
    one = lambda mask, f: imgaug.jitter_reference(u, params([(0, 0, 0)], [mask], f), (13, 17))[0]
    assert (one(B, [0, 1, 1, 0, 1]) == 0).all()
    m = imgaug.gray_mean(imgaug.to_float(u[0]))
    assert 0 < m < 1 and (bits(one(C, [1, 0, 1, 0, 1])) == bits(m)).all()
    g = one(S, [1, 1, 0, 0, 1])
    x = imgaug.to_float(u[0])
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[1], g[2]) and np.array_equal(bits(g[0]), bits(imgaug.gray(x)))
    # the same gray in float64, from the u8 values
    g64 = (0.2989 * u[0, :, :, 0] + 0.587 * u[0, :, :, 1] + 0.114 * u[0, :, :, 2]) / 255.0
    assert np.abs(g[0] - g64).max() < 4e-7


HUE_MEASURED = 8.85e-7


def test_hue_against_colorsys():
    """The hue op against colorsys (float64, the shift applied to h in HSV) on the 17^3 lattice of u8 colours, the 256 grays and 4096 random
    colours, shifts -0.5, -0.05, 0, 0.05, 0.5.  Largest absolute difference measured when this was written: 8.85e-7 (at -0.05; 7.0e-7 at 0 and
    +-0.5, 8.7e-7 at 0.05) -- a few float32 roundings of values in [0, 1].  Asserted: four times that, 3.54e-6, far below 1/510."""
    lat = np.array([min(255, 16 * i) for i in range(17)], dtype=np.uint8)
    cols = np.concatenate([np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), -1).reshape(-1, 3),
                           np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1), noise((4096, 3), 1)])
    bound = 4 * HUE_MEASURED
    assert bound < 1 / 510
    hsv = [colorsys.rgb_to_hsv(*(c / 255.0)) for c in cols]
    worst = 0.0
    for fh in (-0.5, -0.05, 0.0, 0.05, 0.5):
        got = imgaug.apply_ops(cols[None], Hh, [1, 1, 1, fh, 1])[0]
        want = np.array([colorsys.hsv_to_rgb((h + float(np.float32(fh))) % 1.0, s, v) for h, s, v in hsv])
        d = float(np.abs(got.astype(np.float64) - want).max())
        print(f"hue shift {fh}: largest difference from colorsys {d:.3e}")
        worst = max(worst, d)
        assert got.dtype == np.float32 and not np.isnan(got).any()
    assert worst <= bound, worst


def test_contrast_mean_against_float64():
    for u in (noise((33, 47, 3), 3), np.full((20, 31, 3), 255, np.uint8), np.zeros((5, 5, 3), np.uint8), np.full((7, 9, 3), 77, np.uint8),
              noise((1, 1, 3), 4)):
        x = imgaug.to_float(u).astype(np.float64)
        g = 0.2989 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]
        m = imgaug.gray_mean(imgaug.to_float(u))
        assert m.dtype == np.float32 and abs(float(m) - g.mean()) <= 2.0 ** -20
    u = noise((2, 6, 7, 3), 5)
    p = params([(0, 0, 0)] * 2, [C, B | C], [[0.5, 1, 1, 0, 1]] * 2)
    s = imgaug.gray_sum_reference(u, p)
    assert s.dtype == np.uint64 and s[0] == imgaug._gray_sum(imgaug.to_float(u[0]))
    assert s[1] == imgaug._gray_sum(imgaug.blend(imgaug.to_float(u[1]), np.float32(0), 0.5))


def test_sharpness():
    f = [1, 1, 1, 0, 2]
    const = np.full((1, 6, 7, 3), 201, np.uint8)
    got = imgaug.jitter_reference(const, params([(0, 0, 0)], [SH], f), (6, 7))[0]
    v = np.float32(201) / np.float32(255)
    assert np.abs(got - v).max() <= 2 * np.spacing(v)
    u = noise((1, 8, 9, 3), 6)
    x = np.transpose(imgaug.to_float(u[0]), (2, 0, 1))
    got = imgaug.jitter_reference(u, params([(0, 0, 0)], [SH], f), (8, 9))[0]
    for edge in (got[:, 0] == x[:, 0], got[:, -1] == x[:, -1], got[:, :, 0] == x[:, :, 0], got[:, :, -1] == x[:, :, -1]):
        assert edge.all()
    assert (got[:, 1:-1, 1:-1] != x[:, 1:-1, 1:-1]).any()
    # a crop strictly inside: its own edge pixels are sharpened, the border is the source's
    inner = imgaug.jitter_reference(u, params([(2, 1, 0)], [SH], f), (5, 4))[0]
    assert np.array_equal(bits(inner), bits(got[:, 1:6, 2:6]))
    small = noise((1, 2, 5, 3), 7)
    assert np.array_equal(bits(imgaug.jitter_reference(small, params([(0, 0, 0)], [SH], f), (2, 5))[0]), bits(np.transpose(imgaug.to_float(small[0]), (2, 0, 1))))
    # one bright pixel, factor 0 (the blur itself): 5/13 at the pixel, 1/13 at its eight neighbours, 0 elsewhere inside
    dot = np.zeros((1, 7, 7, 3), np.uint8)
    dot[0, 3, 3] = 255
    blur = imgaug.jitter_reference(dot, params([(0, 0, 0)], [SH], [1, 1, 1, 0, 0]), (7, 7))[0, 0]
    want = np.zeros((7, 7))
    want[2:5, 2:5] = 1 / 13
    want[3, 3] = 5 / 13
    assert np.abs(blur - want).max() < 1e-7 and blur[1, 1] == 0 and blur[3, 3] == np.float32(5) / np.float32(13)


def test_plan():
    a = imgaug.augment_plan(2000, None, seed=3, epoch=1, batch=2, camera_index=1)
    b = imgaug.augment_plan(2000, True, seed=3, epoch=1, batch=2, camera_index=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert a[0].dtype == np.int32 and a[1].dtype == np.float32 and a[1].shape == (2000, 5)
    for other in (dict(seed=4, epoch=1, batch=2, camera_index=1), dict(seed=3, epoch=2, batch=2, camera_index=1), dict(seed=3, epoch=1, batch=3, camera_index=1),
                  dict(seed=3, epoch=1, batch=2, camera_index=0)):
        assert not np.array_equal(imgaug.augment_plan(2000, None, **other)[0], a[0])
    mask, fac = a
    nbits = sum((mask >> k) & 1 for k in range(5))
    assert (nbits == 3).all()
    for k, name in enumerate(imgaug.OPS):
        lo, hi = (np.float32(v) for v in imgaug.DEFAULT_CFG[name]["min_max"])
        on = (mask >> k & 1).astype(bool)
        assert ((fac[on, k] >= lo) & (fac[on, k] <= hi)).all() and (fac[~on, k] == imgaug.IDENTITY[k]).all()
        share = on.mean()
        print(f"{name}: chosen for {share:.3f} of 2000 images")
        assert 0.5 <= share <= 0.7           # 60 % expected, sigma about 1.1 %
        assert np.unique(fac[on, k]).size > 1000
    imgaug.check_jitter((1, 8, 8), imgaug.pack_params(np.zeros((2000, 3)), mask, fac), (8, 8), src_index=np.zeros(2000, int))
    # a weight of 0 is never chosen, k follows the ops that are left
    m0, f0 = imgaug.augment_plan(2000, {"hue": {"weight": 0}, "sharpness": {"weight": 0.0}, "max_num_transforms": 2}, seed=5)
    assert not (m0 & (Hh | SH)).any() and (sum((m0 >> k) & 1 for k in range(5)) == 2).all()
    m1, _ = imgaug.augment_plan(50, {"brightness": {"weight": 0}, "contrast": {"weight": 0}, "saturation": {"weight": 0}}, seed=5)
    assert (m1 == (Hh | SH)).all()
    m2, f2 = imgaug.augment_plan(50, {"max_num_transforms": 0})
    assert not m2.any() and (f2 == imgaug.IDENTITY).all()
    m3, f3 = imgaug.augment_plan(300, {"saturation": {"min_max": (0.0, 16.0)}, "max_num_transforms": 5})
    assert (m3 == 31).all() and f3[:, 2].max() > 8
    for bad in ({"hue": {"min_max": (-0.6, 0.1)}}, {"brightness": {"min_max": (0.5, 17)}}, {"contrast": {"weight": -1}}, {"gamma": {}}, {"max_num_transforms": -1},
                {"sharpness": {"min_max": (1.2, 0.8)}}):
        with pytest.raises(ValueError):
            imgaug.augment_plan(4, bad)


def test_plan_leaves_the_epoch_plan_alone():
    sizes = {"a": (16, 24), "b": (24, 32)}

    def same(p, q):
        return len(p) == len(q) and all(np.array_equal(x[0], y[0]) and all(np.array_equal(x[1][c], y[1][c]) for c in sizes) for x, y in zip(p, q))

    before = dataset.epoch_plan(12, 5, sizes, (12, 20), "random", seed=7, epoch=1)
    imgaug.augment_plan(100, None, seed=7, epoch=1, batch=0, camera_index=0)
    after = dataset.epoch_plan(12, 5, sizes, (12, 20), "random", seed=7, epoch=1)
    assert same(before, after)


def test_check_jitter_refuses():
    ok = dict(src_shape=(3, 7, 9), boxes=[(1, 1, 0), (4, 3, 1)], masks=[31, 0], factors=[[1, 1, 1, 0, 1]] * 2, out_hw=(4, 5), mean=None, std=None, src_index=None)

    def check(**kw):
        a = dict(ok, **kw)
        p = (np.asarray(a["boxes"], dtype=np.int32).reshape(-1, 3), a["masks"], a["factors"])
        imgaug.check_jitter(a["src_shape"], params(*p) if len(a["masks"]) else (np.zeros((0, 4), np.int32), np.zeros((0, 5), np.float32)), a["out_hw"],
                            a["mean"], a["std"], a["src_index"])

    check()
    check(mean=[0.5] * 3, std=[0.25] * 3, src_index=[2, 0])
    check(masks=[0, 0], factors=[[np.nan, np.inf, -1, 9, 99]] * 2)          # factors of unset bits are not looked at
    check(factors=[[16, 0, 16, 0.5, 16], [0, 16, 0, -0.5, 0]], masks=[31, 31])
    nan, inf = float("nan"), float("inf")
    refused = [dict(src_shape=(3, 0, 9)), dict(src_shape=(3, 7, 0)), dict(src_shape=(3, 65536, 9)), dict(src_shape=(3, 7, 65536)), dict(out_hw=(0, 5)),
               dict(out_hw=(4, 0)), dict(out_hw=(65536, 5)), dict(out_hw=(4, 65536)), dict(out_hw=(8, 5)), dict(out_hw=(4, 10)),
               dict(boxes=[(5, 1, 0), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 4, 0)]), dict(boxes=[(-1, 0, 0), (0, 0, 0)]), dict(boxes=[(0, -1, 0), (0, 0, 0)]),
               dict(boxes=[(0, 0, 2), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 0, -1)]), dict(masks=[32, 0]), dict(masks=[0, -1]),
               dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(src_shape=(1, 7, 9)), dict(src_shape=(0, 7, 9)), dict(boxes=[], masks=[], factors=[]),
               dict(std=[0.2, 0, 0.2], mean=[0.5] * 3), dict(std=[0.2, nan, 0.2], mean=[0.5] * 3), dict(std=[inf, 0.2, 0.2], mean=[0.5] * 3)]
    for k in range(5):
        for v in (nan, inf, -inf, (0.50001 if k == 3 else 16.001), (-0.50001 if k == 3 else -0.001)):
            f = [1, 1, 1, 0, 1]
            f[k] = v
            refused.append(dict(masks=[0, 1 << k], factors=[[1, 1, 1, 0, 1], f]))
    for kw in refused:
        with pytest.raises(ValueError):
            check(**kw)
