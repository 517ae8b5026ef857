"""av_aloha_amd/imgresize.py, the specification of avsim_image_resize: against torch's CPU interpolate(mode="bilinear", align_corners=False,
antialias=...) on [0, 1] data within 1e-5 -- three times the largest difference a prototype of the specification showed against torch (3.4e-6,
without antialias at 640 -> 224), a bound measured against torch and not against the code under test --, against its own algebra (identity,
constants, boxes, flip), the letterbox plan against the formula restated here, every refusal of check_resize, and that
dataset.TrainingBatches' plans do not depend on the new arguments.  No device needed."""
import types

import numpy as np
import pytest

from av_aloha_amd import dataset, imgresize

SHAPES = [((37, 53), (37, 20)), ((37, 53), (20, 17)), ((48, 64), (17, 23)), ((64, 64), (4, 4)), ((480, 640), (168, 224)), ((30, 40), (45, 61))]
BOUND = 1e-5


def whole(n, H, W, oh, ow, flip=0):
    return np.array([[0, 0, W, H, flip]] * n, dtype=np.int32), np.array([[0, 0, ow, oh]] * n, dtype=np.int32)


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(3).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)


@pytest.mark.parametrize("antialias", [1, 0], ids=["antialias", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_the_reference_against_torch(shape, antialias):
    import torch
    (H, W), (oh, ow) = shape
    u8 = np.random.default_rng(H * 1000 + ow).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    sb, dst = whole(1, H, W, oh, ow)
    got = imgresize.resize_reference(u8, 0, sb, dst, (oh, ow), antialias)
    x = torch.from_numpy(u8).permute(0, 3, 1, 2).to(torch.float32) / 255
    want = torch.nn.functional.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=bool(antialias)).numpy()
    worst = float(np.abs(got - want).max())
    print(f"{shape} antialias {antialias}: largest difference from torch {worst:.3g}")
    assert got.dtype == np.float32 and got.shape == (1, 3, oh, ow) and worst <= BOUND
    # the float format, read as floats: the same bits from the same values
    f = np.ascontiguousarray((u8.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))
    assert np.array_equal(imgresize.resize_reference(f, 1, sb, dst, (oh, ow), antialias), got)


def test_taps_are_the_formula():
    """resize_taps against the docstring's steps in a scalar loop."""
    f = np.float32
    for n_in, n_out, aa in [(53, 20, 1), (53, 20, 0), (40, 61, 1), (64, 4, 1), (7, 7, 1), (1, 1, 1), (65, 4, 0), (5, 1, 1)]:
        lo, count, weight = imgresize.resize_taps(n_in, n_out, aa)
        scale = f(n_in) / f(n_out)
        support, inv = (scale, f(1) / scale) if aa and scale >= 1 else (f(1), f(1))
        assert weight.shape == (n_out, 2 * int(np.ceil(support)) + 1) and weight.dtype == np.float32
        for i in range(n_out):
            center = scale * (f(i) + f(0.5))
            a, b = max(0, int(f(center - support) + f(0.5))), min(n_in, int(f(center + support) + f(0.5)))
            raw = [max(f(0), f(1) - abs(f(f(f(j) - center) + f(0.5)) * inv)) for j in range(a, b)]
            tot = f(0)
            for r in raw:
                tot = f(tot + r)
            assert lo[i] == a and count[i] == b - a
            assert np.array_equal(weight[i, :b - a], np.array([f(r / tot) for r in raw], dtype=np.float32)) and (weight[i, b - a:] == 0).all()
            assert abs(float(weight[i].sum()) - 1) < 1e-6


def test_same_size_is_the_identity(noise):
    H, W = noise.shape[1:3]
    for aa in (0, 1):
        got = imgresize.resize_reference(noise, 0, *whole(2, H, W, H, W), (H, W), aa)
        assert np.array_equal(got, (noise.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2))


def test_a_constant_stays_constant():
    """Within 2 ulp of u / 255, asserted for the filters of at most 7 taps (both settings at ratios up to 3, the same size, an upscale).  A pass
    over n taps rounds n products and n - 1 sums, so what it does to a constant grows with n, and the roundings are the specification's own: at
    ratio 12 (27 taps) and at the cap (33 taps) the antialiased result is 3 and 4 ulp off for u = 1 and 128, which sit at the bottom of a
    binade.  Those two shapes are printed here, not asserted."""
    for value in (1, 77, 128, 255):
        u8 = np.full((1, 48, 64, 3), value, dtype=np.uint8)
        v = np.float32(value) / np.float32(255)
        for (oh, ow) in [(17, 23), (24, 32), (48, 64), (60, 90), (4, 4), (3, 4)]:
            for aa in (0, 1):
                got = imgresize.resize_reference(u8, 0, *whole(1, 48, 64, oh, ow), (oh, ow), aa)
                ulps = float(np.abs(got - v).max() / np.spacing(v))
                taps = max(imgresize.resize_taps(48, oh, aa)[2].shape[1], imgresize.resize_taps(64, ow, aa)[2].shape[1])
                print(f"u = {value}, 48 x 64 -> {oh} x {ow}, antialias {aa}, {taps} taps: {ulps:g} ulp")
                if taps <= 7:
                    assert ulps <= 2


def test_a_box_is_the_cropped_copy_and_flip_flips(noise):
    x0, y0, w, h = 5, 3, 41, 30
    crop = np.ascontiguousarray(noise[:, y0:y0 + h, x0:x0 + w])
    for aa in (0, 1):
        for oh, ow in [(11, 13), (30, 41), (40, 50)]:
            dst = np.array([[0, 0, ow, oh]] * 2, dtype=np.int32)
            boxed = imgresize.resize_reference(noise, 0, np.array([[x0, y0, w, h, 0]] * 2, dtype=np.int32), dst, (oh, ow), aa)
            assert np.array_equal(boxed, imgresize.resize_reference(crop, 0, *whole(2, h, w, oh, ow), (oh, ow), aa))
            flipped = imgresize.resize_reference(noise, 0, np.array([[x0, y0, w, h, 1]] * 2, dtype=np.int32), dst, (oh, ow), aa)
            assert np.array_equal(flipped, boxed[:, :, :, ::-1])


def test_padding_fill_source_index_and_normalisation(noise):
    H, W = noise.shape[1:3]
    oh, ow = 24, 32
    plan = imgresize.resize_with_pad_plan((H, W), (oh, ow))
    ox, oy, rw, rh = plan
    assert (ox, rw) == (0, 32) and oy == oh - rh and rh == int(H / max(W / ow, H / oh))
    fill, mean, std = [0.25, 0.5, 0.75], [0.4, 0.5, 0.6], [0.2, 0.25, 0.3]
    sb = np.array([[0, 0, W, H, 0]] * 3, dtype=np.int32)
    dst = np.array([plan] * 3, dtype=np.int32)
    got = imgresize.resize_reference(noise, 0, sb, dst, (oh, ow), 1, fill, mean, std, [1, 0, 1])
    inner = imgresize.resize_reference(noise, 0, *whole(2, H, W, rh, rw), (rh, rw), 1)
    m, s, f = (np.array(v, dtype=np.float32).reshape(1, 3, 1, 1) for v in (mean, std, fill))
    assert np.array_equal(got[:, :, oy:, :], ((inner - m) / s)[[1, 0, 1]])
    assert np.array_equal(got[:, :, :oy, :], np.broadcast_to((f - m) / s, (3, 3, oy, ow)))
    assert np.array_equal(got[0], got[2])


def test_the_letterbox_plan():
    def formula(H, W, oh, ow):
        ratio = max(W / ow, H / oh)
        rw, rh = int(W / ratio), int(H / ratio)
        return ow - rw, oh - rh, rw, rh

    assert imgresize.resize_with_pad_plan((480, 640), (224, 224)) == (0, 56, 224, 168)
    assert imgresize.resize_with_pad_plan((480, 640), (224, 224), "center") == (0, 28, 224, 168)
    for (H, W), (oh, ow) in [((480, 640), (224, 224)), ((432, 576), (512, 512)), ((640, 480), (224, 224)), ((37, 53), (24, 32)), ((16, 24), (24, 32)), ((100, 100), (96, 96))]:
        px, py, rw, rh = formula(H, W, oh, ow)
        assert imgresize.resize_with_pad_plan((H, W), (oh, ow)) == (px, py, rw, rh)
        assert imgresize.resize_with_pad_plan((H, W), (oh, ow), "center") == (px // 2, py // 2, rw, rh)
        assert 1 <= rw <= ow and 1 <= rh <= oh and (rw == ow or rh == oh)
    with pytest.raises(ValueError):
        imgresize.resize_with_pad_plan((480, 640), (224, 224), "bottom")


def test_every_refusal():
    ok = dict(src_shape=(3, 64, 80), src_box=[(0, 0, 80, 64, 0), (8, 8, 64, 48, 1)], dst=[(0, 0, 20, 16), (2, 3, 10, 8)], src_index=None, out_hw=(16, 20), fmt=0,
              antialias=1, fill=None, mean=None, std=None)
    imgresize.check_resize(**ok)
    imgresize.check_resize(**dict(ok, src_index=[2, 0], fill=[0.1, 0.2, 0.3], mean=[0.5] * 3, std=[0.25] * 3, antialias=0, fmt=1))
    imgresize.check_resize(**dict(ok, src_box=[(0, 0, 80, 64, 0), (0, 0, 80, 64, 0)], dst=[(0, 0, 5, 4), (0, 0, 20, 16)]))          # the ratio cap itself
    nan, inf = float("nan"), float("inf")
    refused = [dict(fmt=2), dict(fmt=-1), dict(src_shape=(3, 0, 80)), dict(src_shape=(3, 64, 65536)), dict(out_hw=(0, 20)), dict(out_hw=(16, 65536)),
               dict(src_shape=(0, 64, 80)), dict(src_box=[], dst=[]),
               dict(src_box=[(0, 0, 81, 64, 0), (0, 0, 80, 64, 0)]), dict(src_box=[(0, 1, 80, 64, 0), (0, 0, 80, 64, 0)]), dict(src_box=[(-1, 0, 80, 64, 0), (0, 0, 80, 64, 0)]),
               dict(src_box=[(0, -1, 80, 64, 0), (0, 0, 80, 64, 0)]),
               dict(dst=[(1, 0, 20, 16), (0, 0, 20, 16)]), dict(dst=[(0, 1, 20, 16), (0, 0, 20, 16)]), dict(dst=[(-1, 0, 20, 16), (0, 0, 20, 16)]), dict(dst=[(0, -1, 20, 15), (0, 0, 20, 16)]),
               dict(src_box=[(0, 0, 0, 64, 0), (0, 0, 80, 64, 0)]), dict(src_box=[(0, 0, 80, 0, 0), (0, 0, 80, 64, 0)]), dict(dst=[(0, 0, 0, 16), (0, 0, 20, 16)]),
               dict(dst=[(0, 0, 20, 0), (0, 0, 20, 16)]), dict(src_box=[(0, 0, -3, 64, 0), (0, 0, 80, 64, 0)]),
               dict(dst=[(0, 0, 4, 16), (0, 0, 20, 16)]), dict(dst=[(0, 0, 20, 3), (0, 0, 20, 16)]),                                   # 80 / 4 and 64 / 3: above 16
               dict(src_box=[(0, 0, 80, 64, 2), (0, 0, 80, 64, 0)]), dict(src_box=[(0, 0, 80, 64, 0), (0, 0, 80, 64, -1)]), dict(antialias=2), dict(antialias=-1),
               dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(src_shape=(1, 64, 80)),
               dict(fill=[0, nan, 0]), dict(fill=[inf, 0, 0]), dict(mean=[0.5] * 3, std=[0.2, 0, 0.2]), dict(mean=[0.5] * 3, std=[nan, 0.2, 0.2]),
               dict(mean=[0.5] * 3, std=[0.2, 0.2, inf]), dict(mean=[0.5] * 3), dict(std=[0.5] * 3)]
    for kw in refused:
        with pytest.raises(ValueError):
            imgresize.check_resize(**dict(ok, **kw))
    with pytest.raises(ValueError):          # 16.1 : 1
        imgresize.resize_reference(np.zeros((1, 161, 20, 3), dtype=np.uint8), 0, [(0, 0, 20, 161, 0)], [(0, 0, 20, 10)], (10, 20))
    with pytest.raises(ValueError):          # the format has to be the array's
        imgresize.resize_reference(np.zeros((1, 16, 20, 3), dtype=np.uint8), 1, [(0, 0, 20, 16, 0)], [(0, 0, 20, 10)], (10, 20))


def test_training_plans_do_not_depend_on_resize():
    """TrainingBatches(resize=None) -- and with a resize -- plans what a TrainingBatches built without the argument plans: the same frames, the
    same boxes, the same augmentation draws."""
    import torch
    cams = {"cam_a": (16, 24), "cam_b": (24, 32)}
    ds = types.SimpleNamespace(torch=torch, cameras=list(cams), size=cams, n=12, device="cpu")
    stats = {f"observation.images.{c}": {"mean": np.full((3, 1, 1), 0.5, np.float32), "std": np.full((3, 1, 1), 0.25, np.float32)} for c in cams}
    stats["observation.state"] = stats["action"] = {"mean": np.zeros(3, np.float32), "std": np.ones(3, np.float32)}
    for kw in (dict(crop=(12, 20), seed=7), dict(crop=None, crop_mode="center", seed=2, drop_last=False), dict(crop=(12, 20), seed=4, augment=True),
               dict(crop=(12, 20), seed=5, n_obs_steps=2)):
        old = dataset.TrainingBatches(ds, 5, 4, stats, **kw)
        for extra in (dict(resize=None), dict(resize=(24, 32), resize_mode="pad"), dict(resize=(8, 8), antialias=False)):
            new = dataset.TrainingBatches(ds, 5, 4, stats, **kw, **extra)
            for epoch in range(2):
                a, b = old.plan(epoch), new.plan(epoch)
                assert len(a) == len(b) == len(dataset.epoch_plan(12, 5, cams, kw.get("crop"), kw.get("crop_mode", "random"), kw["seed"], epoch, kw.get("drop_last", True)))
                for (pa, ba), (pb, bb) in zip(a, b):
                    assert np.array_equal(pa, pb) and all(np.array_equal(ba[c], bb[c]) for c in cams)
                pa, pb = old.augment_plan(epoch), new.augment_plan(epoch)
                assert (pa is None) == (pb is None)
                if pa is not None:
                    for x, y in zip(pa, pb):
                        assert all(np.array_equal(u, v) for c in cams for u, v in zip(x[c], y[c]))
        none = dataset.TrainingBatches(ds, 5, 4, stats, **kw, resize=None)
        assert none.resize is None and set(none.mean_std) == set(old.mean_std)
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 5, 4, stats, resize=(24, 32), resize_mode="fit")
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 5, 4, stats, resize=(1, 32))          # 16 rows -> 1 is fine, 24 rows -> 1 is above the cap
    with pytest.raises(ValueError):
        dataset.TrainingBatches(ds, 5, 4, stats, resize=(0, 32))
