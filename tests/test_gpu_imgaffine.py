"""The device's geometric augmentation (avsim_image_augment, csrc/avsim_imgaug.hip: k_aug_affine, k_aug_whole, k_aug_apply_list) against its
specification, av_aloha_amd/imgaug.py (jitter_affine_reference).  Every comparison is np.array_equal on the float32 arrays with no NaN in
either -- equality of bits, -0 and +0 aside -- through a host-pointer handle and a device handle.  Inputs: noise u8 images with fixed seeds.
The tile is 16 rows x 64 columns, so the large image is 35 x 133: three tiles each way, neither side a multiple of the tile or of 4; nsrc = 3,
so images 1 and 2 start off a 16-byte boundary wherever 3 H W % 16 != 0."""
import numpy as np
import pytest

from av_aloha_amd import _ffi, imgaug
from avsim_test_util import noise
from gpu_util import Guarded, torch as T
from gpu_util import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

AFFINE = 32
SENTINEL = 0xA5A5A5A5 - (1 << 32)      # as an int32
LARGE = (2 * 16 + 3, 2 * 64 + 5)
SIZES = [(1, 1), (2, 5), (3, 3), (5, 67), LARGE]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
FAC_A, FAC_B = [0.8, 1.2, 1.5, 0.05, 1.2], [1.2, 0.8, 0.5, -0.05, 2.0]
SCRATCH_DEFAULT = float(128 << 20)


def matrices(H, W):
    """float32 [10, 6]: the identity, an integer shift, a shift out of the image, 90 and 180 degrees, +-5 degrees with a translation, 45 degrees
    at scale 0.5 and 2, a sheared one."""
    m = imgaug.affine_matrix
    return np.stack([m(0), m(0, 3, -2), m(0, W + 1, 0), m(90), m(180), m(5, 2, 1), m(-5, -1, 2), m(45, 0, 0, 0.5), m(45, 1, 0, 2.0), m(10, 1, -1, 1.1, 8, -4)])


def boxes_for(H, W):
    """[(out_hw, boxes)]: the whole image; a crop two smaller each way where the image allows, at every combination of first / middle / last
    position: on each of the four borders, and at (1, 1) strictly inside.  Each with flip 0 and 1."""
    out = [((H, W), [(0, 0, 0), (0, 0, 1)])]
    ch, cw = (H - 2 if H >= 3 else H), (W - 2 if W >= 3 else W)
    if (ch, cw) != (H, W):
        xs, ys = sorted({0, (W - cw) // 2, W - cw}), sorted({0, (H - ch) // 2, H - ch})
        out.append(((ch, cw), [(x, y, f) for y in ys for x in xs for f in (0, 1)]))
    return out


def dev_augment(dev, t_img, shape, bm, fac, mat, interp, si, ms, out_hw, guard, nout=None):
    """avsim_image_augment through the device handle into the middle of a sentinel-filled tensor -> (rc, out, no word around it was
    written, none of it was written)."""
    h, d = dev
    n, H, W = shape
    oh, ow = out_hw
    size = len(bm) * 3 * max(oh, 0) * max(ow, 0) if 0 < oh < 65536 and 0 < ow < 65536 else 64
    g = Guarded(d, size, T.int32, SENTINEL, guard, 1024)
    rc = h.L.avsim_image_augment(h.h, t_img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(mat), interp, _ffi.ptr(si), len(bm) if nout is None else nout,
                                 _ffi.ptr(ms), oh, ow, g.ptr())
    T.cuda.synchronize()
    out, intact, untouched = g.read()
    return rc, out.view(np.uint32), intact, untouched


_case = [0]


def both_equal_the_reference(sim, dev, u8, boxes, masks, factors, mats, interp, out_hw, src_index=None, normalise=True, what=""):
    """One call through each handle against imgaug.jitter_affine_reference."""
    bm, fac = imgaug.pack_params(boxes, masks, factors)
    mat = None if mats is None else np.ascontiguousarray(mats, dtype=np.float32).reshape(len(bm), 6)
    si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32)
    mean, std = (MEAN, STD) if normalise else (None, None)
    want = imgaug.jitter_affine_reference(u8, (bm, fac), mat, interp, out_hw, mean, std, si)
    assert not np.isnan(want).any()
    got = sim.augment_images(u8, (bm, fac), mat, out_hw, interp, mean, std, si)
    assert got.dtype == np.float32 and not np.isnan(got).any() and np.array_equal(got, want), f"host mode: {what}"
    guard = 1024 if _case[0] % 2 == 0 else 1021                                # `out` on and off a 16-byte boundary
    _case[0] += 1
    rc, out, intact, _ = dev_augment(dev, T.from_numpy(u8).to(dev[1]), u8.shape[:3], bm, fac, mat, interp, si, imgaug.mean_std(mean, std), out_hw, guard)
    out = out.view(np.float32).reshape(want.shape)
    assert rc == 0 and not np.isnan(out).any() and np.array_equal(out, want), f"device mode: {what}"
    assert intact, f"device mode: {what}: bytes outside `out` were written"
    return got


def spread(boxes, nsrc, choices):
    """Every box with every choice (mask, factors, matrix): boxes, masks, factors, matrices, src_index (the sources in turn)."""
    b, m, f, a = [], [], [], []
    for mask, fac, mat in choices:
        for box in boxes:
            b.append(box), m.append(mask), f.append(fac), a.append(mat)
    return np.array(b, dtype=np.int32), np.array(m, dtype=np.int32), np.array(f, dtype=np.float32), np.array(a, dtype=np.float32), np.arange(len(b), dtype=np.int32) % nsrc


@pytest.mark.parametrize("interp", [0, 1], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_affine_op_alone(sim, dev, size, interp):
    """Mask 32 with every matrix, on every box (each border, strictly inside, both flips), with and without mean / std."""
    H, W = size
    u8 = noise((3, H, W, 3), 100 * H + W)
    choices = [(AFFINE, [3.0, 3.0, 3.0, 0.25, 3.0], M) for M in matrices(H, W)]         # the factors of unset bits are not looked at
    for n, (out_hw, boxes) in enumerate(boxes_for(H, W)):
        b, m, f, a, si = spread(boxes, 3, choices)
        got = both_equal_the_reference(sim, dev, u8, b, m, f, a, interp, out_hw, si, normalise=n % 2 == 0, what=f"affine alone, {out_hw}")
        if n == 1:                                                              # no mean / std: the shift out of the image is all fill
            assert all((got[i] == 0).all() for i in range(2 * len(boxes), 3 * len(boxes)))


@pytest.mark.parametrize("interp", [0, 1], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_affine_after_the_colour_ops(sim, dev, size, interp):
    """32 with each single colour op, 48 (sharpness + affine: through the scratch images) and 63, the matrices in turn."""
    H, W = size
    u8 = noise((3, H, W, 3), 300 * H + W)
    mats = matrices(H, W)
    masks = [33, 34, 36, 40, 48, 63, 63, 48]
    choices = [(mask, FAC_A if k % 2 == 0 else FAC_B, mats[(3 * k + j) % len(mats)]) for k, mask in enumerate(masks) for j in range(3)]
    for n, (out_hw, boxes) in enumerate(boxes_for(H, W)):
        b, m, f, a, si = spread(boxes[::5] if len(boxes) > 2 else boxes, 3, choices)
        both_equal_the_reference(sim, dev, u8, b, m, f, a, interp, out_hw, si, normalise=n % 2 == 1, what=f"colour ops + affine, {out_hw}")
    # NULL src_index: output i reads image i
    b = np.array([(0, 0, 0), (0, 0, 1), (0, 0, 0)], dtype=np.int32)
    both_equal_the_reference(sim, dev, u8, b, [63, 48, 34], [FAC_A] * 3, mats[[5, 6, 9]], interp, (H, W), None, True, what="no src_index")


@pytest.mark.parametrize("interp", [0, 1], ids=["nearest", "bilinear"])
def test_a_batch_that_mixes_masks(sim, dev, interp):
    """Outputs with and without bit 5, with and without contrast and sharpness in one call; sources shared, repeated and permuted."""
    H, W = LARGE
    u8 = noise((3, H, W, 3), 41)
    masks = np.array([0, 32, 2, 34, 16, 48, 63, 31, 40, 18, 50, 32, 12, 44], dtype=np.int32)
    n = len(masks)
    src_index = np.array([2, 2, 0, 1, 1, 0, 2, 0, 1, 2, 2, 2, 0, 0], dtype=np.int32)
    rng = np.random.default_rng(42)
    fac = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), rng.uniform(0, 2, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0, 2, n)], axis=1).astype(np.float32)
    mats = np.stack([imgaug.affine_matrix(rng.uniform(-30, 30), rng.integers(-6, 7), rng.integers(-3, 4), rng.uniform(0.8, 1.25), rng.uniform(-5, 5)) for _ in range(n)])
    mats[~(masks & AFFINE).astype(bool)] = np.nan                               # the entries of outputs without bit 5 are not read
    oh, ow = 21, 90
    boxes = np.stack([rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n)], axis=1).astype(np.int32)
    for normalise in (True, False):
        both_equal_the_reference(sim, dev, u8, boxes, masks, fac, mats, interp, (oh, ow), src_index, normalise, what="mixed masks")


def test_without_bit_5_the_call_is_image_jitter(sim, dev):
    """The same call with no bit 5 equals avsim_image_jitter's output bit for bit, with matrices given and with NULL."""
    H, W = LARGE
    u8 = noise((3, H, W, 3), 43)
    rng = np.random.default_rng(44)
    n = 32
    masks = np.arange(32, dtype=np.int32)
    fac = np.stack([rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n), rng.uniform(0, 2, n), rng.uniform(-0.5, 0.5, n), rng.uniform(0, 2, n)], axis=1).astype(np.float32)
    oh, ow = 30, 131
    boxes = np.stack([rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n)], axis=1).astype(np.int32)
    si = rng.integers(0, 3, n).astype(np.int32)
    bm, fac = imgaug.pack_params(boxes, masks, fac)
    old = sim.jitter_images(u8, (bm, fac), (oh, ow), MEAN, STD, si)
    assert np.array_equal(old, imgaug.jitter_reference(u8, (bm, fac), (oh, ow), MEAN, STD, si))
    for mat in (None, np.full((n, 6), np.nan, dtype=np.float32)):
        for interp in (0, 1):
            new = sim.augment_images(u8, (bm, fac), mat, (oh, ow), interp, MEAN, STD, si)
            assert np.array_equal(new.view(np.uint32), old.view(np.uint32))
            rc, out, intact, _ = dev_augment(dev, T.from_numpy(u8).to(dev[1]), u8.shape[:3], bm, fac, mat, interp, si, imgaug.mean_std(MEAN, STD), (oh, ow), 1024)
            assert rc == 0 and np.array_equal(out, old.view(np.uint32).reshape(-1)) and intact


def test_refusals_leave_out_untouched(sim, dev):
    H, W, oh, ow = 7, 9, 4, 5
    u8 = noise((3, H, W, 3), 21)
    t_img = T.from_numpy(u8).to(dev[1])
    L = sim.h.L
    eye = [1, 0, 0, 0, 1, 0]
    ok = dict(nsrc=3, h=H, w=W, boxes=[(1, 1, 0), (4, 3, 1)], masks=[63, 32], factors=[[1, 1, 1, 0, 1]] * 2, matrix=[eye, list(imgaug.affine_matrix(20, 1, 0))], interp=1,
              nout=None, src_index=None, out_h=oh, out_w=ow, mean_std=None)

    def arrays(a):
        bm = np.ascontiguousarray(np.concatenate([np.asarray(a["boxes"], dtype=np.int32).reshape(-1, 3), np.asarray(a["masks"], dtype=np.int32).reshape(-1, 1)], axis=1))
        fac = np.ascontiguousarray(a["factors"], dtype=np.float32).reshape(-1, 5)
        mat = None if a["matrix"] is None else np.ascontiguousarray(a["matrix"], dtype=np.float32).reshape(-1, 6)
        si = None if a["src_index"] is None else np.array(a["src_index"], dtype=np.int32)
        ms = None if a["mean_std"] is None else np.array(a["mean_std"], dtype=np.float32)
        return bm, fac, mat, si, ms

    def reference(a):
        bm, fac, mat, si, ms = arrays(a)
        return imgaug.jitter_affine_reference(u8, (bm, fac), mat, a["interp"], (oh, ow), *((ms[0], ms[1]) if ms is not None else (None, None)), si)

    def host(**kw):
        a = dict(ok, **kw)
        bm, fac, mat, si, ms = arrays(a)
        out = np.full((2, 3, oh, ow), 12345.0, dtype=np.float32)
        rc = L.avsim_image_augment(sim.h.h, u8.ctypes.data, a["nsrc"], a["h"], a["w"], bm.ctypes.data, fac.ctypes.data, _ffi.ptr(mat), a["interp"], _ffi.ptr(si),
                                   len(bm) if a["nout"] is None else a["nout"], _ffi.ptr(ms), a["out_h"], a["out_w"], out.ctypes.data)
        if rc:
            assert (out == np.float32(12345.0)).all(), "a refused call wrote `out`"
            assert rc != -1 or len(L.avsim_last_error(sim.h.h)) > 0
        else:
            assert np.array_equal(out, reference(a))
        return rc

    def device(**kw):
        a = dict(ok, **kw)
        bm, fac, mat, si, ms = arrays(a)
        rc, out, intact, untouched = dev_augment(dev, t_img, (a["nsrc"], a["h"], a["w"]), bm, fac, mat, a["interp"], si, ms, (a["out_h"], a["out_w"]), 1024, a["nout"])
        assert intact
        assert untouched if rc else np.array_equal(out.view(np.float32).reshape(2, 3, oh, ow), reference(a)), "a refused call wrote `out`"
        assert rc != -1 or len(dev[0].L.avsim_last_error(dev[0].h)) > 0
        return rc

    nan, inf, big = float("nan"), float("inf"), float(2 ** 20)
    assert host() == 0 and device() == 0
    assert host(mean_std=[[0.5] * 3, [0.25] * 3], src_index=[2, 0], interp=0) == 0
    assert host(masks=[31, 32], matrix=[[nan, inf, -inf, 1e30, nan, nan], eye]) == 0                 # entries of unset bits are not read
    assert host(masks=[32, 32], factors=[[nan, inf, -1, 9, 99]] * 2) == 0                              # factors of unset bits are not looked at
    assert host(matrix=[[big, 0, 0, 0, -big, 0], [0, 0, big, 0, 0, -big]]) == 0 and device(matrix=[[big, 0, 0, 0, -big, 0], [0, 0, big, 0, 0, -big]]) == 0
    assert host(masks=[31, 0], matrix=None) == 0 and device(masks=[31, 0], matrix=None) == 0           # no bit 5: affine may be NULL
    refused = [dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(out_h=0), dict(out_w=0), dict(out_h=65536), dict(out_w=65536),
               dict(nout=0), dict(nout=-1), dict(nsrc=0), dict(nsrc=-1),
               dict(boxes=[(5, 1, 0), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 4, 0)]), dict(boxes=[(-1, 0, 0), (0, 0, 0)]), dict(boxes=[(0, -1, 0), (0, 0, 0)]),
               dict(out_h=8), dict(out_w=10),
               dict(boxes=[(0, 0, 2), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 0, -1)]), dict(masks=[64, 0]), dict(masks=[0, -1]), dict(masks=[0, 127]),
               dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(nsrc=1),
               dict(mean_std=[[0.5] * 3, [0.2, 0, 0.2]]), dict(mean_std=[[0.5] * 3, [nan, 0.2, 0.2]]), dict(mean_std=[[0.5] * 3, [0.2, 0.2, inf]]),
               dict(interp=2), dict(interp=-1), dict(matrix=None), dict(masks=[0, 32], matrix=None)]
    for k in range(5):
        for v in (nan, inf, (0.50001 if k == 3 else 16.001), (-0.50001 if k == 3 else -0.001)):
            f = [1, 1, 1, 0, 1]
            f[k] = v
            refused.append(dict(masks=[32, 32 | 1 << k], factors=[[1, 1, 1, 0, 1], f]))
    for k in range(6):
        for v in (nan, inf, -inf, big * 1.001, -big * 1.001):
            m = list(eye)
            m[k] = v
            refused.append(dict(matrix=[eye, m]))
    for kw in refused:
        assert host(**kw) == -1, kw
        assert device(**kw) == -1, kw
    assert host() == 0 and device() == 0                                      # and the handles still compute the specification
    # avsim_image_jitter keeps refusing bit 5
    bm, fac, mat, si, ms = arrays(ok)
    out = np.full((2, 3, oh, ow), 12345.0, dtype=np.float32)
    assert L.avsim_image_jitter(sim.h.h, u8.ctypes.data, 3, H, W, bm.ctypes.data, fac.ctypes.data, None, 2, None, oh, ow, out.ctypes.data) == -1 and (out == np.float32(12345.0)).all()
    with pytest.raises(ValueError):
        sim.augment_images(u8, (bm, fac), None, (oh, ow))
    with pytest.raises(ValueError):
        sim.augment_images(u8, (bm, fac), mat, (oh, ow), interp=3)


def test_calls_in_a_row_and_more_than_one_scratch_group(dev):
    """Six calls without a synchronisation between them, the caller's arrays overwritten as soon as a call returns (more calls than staging
    slots), each with several sharpness + affine outputs while the scratch cap holds two images: three groups or more per call, the next
    group's fill ordered behind the previous group's gather by the stream alone."""
    h, d = dev
    H, W, oh, ow, n = 33, 130, 20, 64, 9
    h.check(h.L.avsim_set_option(h.h, b"augment_scratch_bytes", float(2 * 12 * H * W + 100)))
    try:
        u8 = noise((n, H, W, 3), 31)
        t_img = T.from_numpy(u8).to(d)
        rng = np.random.default_rng(32)
        bm, fac, si, ms = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 5), dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros((2, 3), dtype=np.float32)
        mat = np.zeros((n, 6), dtype=np.float32)
        outs, wants = [], []
        for k in range(6):
            bm[:, 0], bm[:, 1], bm[:, 2], bm[:, 3] = rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n), rng.integers(0, 64, n)
            bm[:6, 3] |= 48                                                     # at least six outputs through the scratch images
            fac[:] = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n), rng.uniform(0.5, 1.5, n), rng.uniform(-0.05, 0.05, n), rng.uniform(0.8, 1.2, n)], axis=1)
            mat[:] = np.stack([imgaug.affine_matrix(rng.uniform(-20, 20), rng.integers(-6, 7), rng.integers(-2, 3), rng.uniform(0.8, 1.25)) for _ in range(n)])
            si[:] = rng.integers(0, n, n)
            ms[0], ms[1] = rng.uniform(0.3, 0.6, 3), rng.uniform(0.2, 0.3, 3)
            wants.append(imgaug.jitter_affine_reference(u8, (bm.copy(), fac.copy()), mat.copy(), k % 2, (oh, ow), ms[0].copy(), ms[1].copy(), si.copy()))
            out = T.empty((n, 3, oh, ow), dtype=T.float32, device=d)
            h.check(h.L.avsim_image_augment(h.h, t_img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, mat.ctypes.data, k % 2, si.ctypes.data, n, ms.ctypes.data, oh, ow,
                                            out.data_ptr()))
            bm[:], fac[:], mat[:], si[:], ms[:] = 0, 0, 7, 0, 1                 # the caller's arrays are its own again
            outs.append(out)
        T.cuda.synchronize()
        for k in range(6):
            got = outs[k].cpu().numpy()
            assert not np.isnan(got).any() and np.array_equal(got, wants[k]), f"call {k}"
        assert h.L.avsim_set_option(h.h, b"augment_scratch_bytes", 0.0) == -1
    finally:
        h.check(h.L.avsim_set_option(h.h, b"augment_scratch_bytes", SCRATCH_DEFAULT))


def test_the_layers_agree_with_the_reference(sim):
    """DeviceImages.augment_images (tensors, torch's stream) and BatchedSim.augment_images (numpy) on a small batch."""
    from av_aloha_amd.images import DeviceImages
    H, W, oh, ow = 20, 70, 17, 66
    u8 = noise((2, H, W, 3), 61)
    p = np.zeros(3, dtype=imgaug.PARAMS_DTYPE)
    p["x0"], p["y0"], p["flip"], p["mask"] = [0, 3, 4], [1, 0, 3], [0, 1, 1], [63, 34, 24]
    p["factor"] = [[1.1, 0.9, 1.4, 0.03, 1.2], [1, 1.2, 1, 0, 1], [1, 1, 1, -0.2, 0.5]]
    mats = np.stack([imgaug.affine_matrix(5, 3, -1), imgaug.affine_matrix(-5, -2, 1, 1.1), imgaug.IDENTITY_MATRIX])
    si = [1, 0, 1]
    for interp in (0, 1):
        want = imgaug.jitter_affine_reference(u8, p, mats, interp, (oh, ow), MEAN, STD, si)
        assert np.array_equal(sim.augment_images(u8, p, mats, (oh, ow), interp, MEAN, STD, si), want)
    di = DeviceImages()
    try:
        t_img = T.from_numpy(u8).to(di.device)
        got = di.augment_images(t_img, p, mats, (oh, ow), 1, MEAN, STD, si)
        assert got.device == di.device and tuple(got.shape) == (3, 3, oh, ow)
        assert np.array_equal(got.cpu().numpy(), want)
        out = T.empty((3, 3, oh, ow), dtype=T.float32, device=di.device)
        assert di.augment_images(t_img, imgaug.split_params(p), mats, (oh, ow), src_index=si, out=out) is out
        assert np.array_equal(out.cpu().numpy(), imgaug.jitter_affine_reference(u8, p, mats, 0, (oh, ow), src_index=si))
        with pytest.raises(ValueError):
            di.augment_images(t_img, p, mats, (oh + 4, ow), 0, MEAN, STD, si)
    finally:
        di.close()
