"""The device's colour and sharpness augmentation (avsim_image_jitter, csrc/avsim_imgaug.hip) against its specification,
av_aloha_amd/imgaug.py.  Every comparison is np.array_equal on the float32 arrays with no NaN in either -- equality of bits, -0 and +0 aside --
through a host-pointer handle and a device handle.  Inputs: noise u8 images with fixed seeds.  k_aug_apply's tile is 16 rows x 64 columns
(IAG_TY x IAG_TX), so the large image is (2 * 16 + 3) x (2 * 64 + 5) = 35 x 133: three tiles each way, neither side a multiple of the tile or
of 4.  nsrc = 3, so images 1 and 2 start off a 16-byte boundary wherever 3 H W % 16 != 0."""
import numpy as np
import pytest

from av_aloha_amd import _ffi, imgaug
from avsim_test_util import noise
from gpu_util import Guarded, torch as T
from gpu_util import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5 - (1 << 32)      # as an int32
TILE_Y, TILE_X = 16, 64
LARGE = (2 * TILE_Y + 3, 2 * TILE_X + 5)
SIZES = [(1, 1), (2, 5), (3, 3), (5, 67), LARGE]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
# the LeRobot range ends, 0, 1, 2; hue: its range ends, 0 and +-0.5
FACTORS = {0: [0.8, 1.2, 0, 1, 2], 1: [0.8, 1.2, 0, 1, 2], 2: [0.5, 1.5, 0, 1, 2], 3: [-0.05, 0.05, 0, -0.5, 0.5], 4: [0.8, 1.2, 0, 1, 2]}


def boxes_for(H, W):
    """[(out_hw, boxes)]: the whole image; a crop two smaller each way where the image allows (x0 = 1 is odd, W - 2 is no multiple of 4 for
    every W of SIZES) at every combination of first / middle / last position: it touches each of the four source borders, and at (1, 1) lies
    strictly inside, its halo outside the crop but inside the source.  Each with flip 0 and 1."""
    out = [((H, W), [(0, 0, 0), (0, 0, 1)])]
    ch, cw = (H - 2 if H >= 3 else H), (W - 2 if W >= 3 else W)
    if (ch, cw) != (H, W):
        assert cw % 4 != 0
        xs, ys = sorted({0, (W - cw) // 2, W - cw}), sorted({0, (H - ch) // 2, H - ch})
        out.append(((ch, cw), [(x, y, f) for y in ys for x in xs for f in (0, 1)]))
    return out


def dev_jitter(dev, t_img, shape, bm, fac, si, ms, out_hw, guard, nout=None):
    """avsim_image_jitter through the device handle into the middle of a sentinel-filled tensor -> (rc, out, no word around it was
    written, none of it was written)."""
    h, d = dev
    n, H, W = shape
    oh, ow = out_hw
    size = len(bm) * 3 * max(oh, 0) * max(ow, 0) if 0 < oh < 65536 and 0 < ow < 65536 else 64
    g = Guarded(d, size, T.int32, SENTINEL, guard, 1024)
    rc = h.L.avsim_image_jitter(h.h, t_img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(si), len(bm) if nout is None else nout,
                                _ffi.ptr(ms), oh, ow, g.ptr())
    T.cuda.synchronize()
    out, intact, untouched = g.read()
    return rc, out.view(np.uint32), intact, untouched


_case = [0]


def both_equal_the_reference(sim, dev, u8, boxes, masks, factors, out_hw, src_index=None, normalise=True, what=""):
    """One call through each handle against imgaug.jitter_reference."""
    bm, fac = imgaug.pack_params(boxes, masks, factors)
    si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32)
    mean, std = (MEAN, STD) if normalise else (None, None)
    want = imgaug.jitter_reference(u8, (bm, fac), out_hw, mean, std, si)
    assert not np.isnan(want).any()
    got = sim.jitter_images(u8, (bm, fac), out_hw, mean, std, si)
    assert got.dtype == np.float32 and not np.isnan(got).any() and np.array_equal(got, want), f"host mode: {what}"
    guard = 1024 if _case[0] % 2 == 0 else 1021                                # `out` on and off a 16-byte boundary
    _case[0] += 1
    rc, out, intact, _ = dev_jitter(dev, T.from_numpy(u8).to(dev[1]), u8.shape[:3], bm, fac, si, imgaug.mean_std(mean, std), out_hw, guard)
    out = out.view(np.float32).reshape(want.shape)
    assert rc == 0 and not np.isnan(out).any() and np.array_equal(out, want), f"device mode: {what}"
    assert intact, f"device mode: {what}: bytes outside `out` were written"
    return got


def spread(boxes, nsrc, choices):
    """Every box with every choice (mask, factors): boxes, masks, factors, src_index (the sources in turn)."""
    b, m, f = [], [], []
    for mask, fac in choices:
        for box in boxes:
            b.append(box), m.append(mask), f.append(fac)
    return np.array(b, dtype=np.int32), np.array(m, dtype=np.int32), np.array(f, dtype=np.float32), np.arange(len(b), dtype=np.int32) % nsrc


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_single_op_equals_the_reference(sim, dev, size):
    H, W = size
    u8 = noise((3, H, W, 3), 100 * H + W)
    for k in range(5):
        choices = []
        for v in FACTORS[k]:
            f = [3.0, 3.0, 3.0, 0.25, 3.0]                                       # the factors of unset bits are not looked at
            f[k] = v
            choices.append((1 << k, f))
        for n, (out_hw, boxes) in enumerate(boxes_for(H, W)):
            b, m, f, si = spread(boxes, 3, choices)
            both_equal_the_reference(sim, dev, u8, b, m, f, out_hw, si, normalise=(k + n) % 2 == 0, what=f"{imgaug.OPS[k]}, {out_hw}")


def test_all_masks_on_a_small_image(sim, dev):
    H, W = 5, 67
    u8 = noise((3, H, W, 3), 7)
    rng = np.random.default_rng(8)
    choices = [(mask, [FACTORS[k][rng.integers(0, 5)] for k in range(5)]) for mask in range(32)]
    for normalise, (out_hw, boxes) in zip((True, False), boxes_for(H, W)):
        b, m, f, si = spread(boxes[::3] if len(boxes) > 2 else boxes, 3, choices)
        both_equal_the_reference(sim, dev, u8, b, m, f, out_hw, si, normalise, what=f"all masks, {out_hw}")


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_full_chain(sim, dev, size):
    H, W = size
    u8 = noise((3, H, W, 3), 300 * H + W)
    choices = [(31, [0.8, 1.2, 1.5, 0.05, 1.2]), (31, [1.2, 0.8, 0.5, -0.05, 0.8]), (31, [2, 2, 2, 0.5, 2]), (31, [1.2, 0, 2, -0.5, 0])]
    for normalise in (True, False):
        for out_hw, boxes in boxes_for(H, W):
            b, m, f, si = spread(boxes, 3, choices)
            both_equal_the_reference(sim, dev, u8, b, m, f, out_hw, si, normalise, what=f"full chain, {out_hw}")
    # NULL src_index: output i reads image i
    b = np.array([(0, 0, 0), (0, 0, 1), (0, 0, 0)], dtype=np.int32)
    both_equal_the_reference(sim, dev, u8, b, [31, 31, 31], [choices[0][1]] * 3, (H, W), None, True, what="full chain, no src_index")


def test_a_batch_that_mixes_masks(sim, dev):
    """Outputs with and without the contrast bit in one call (the reduction runs for the former only), sources repeated and permuted,
    nout > nsrc."""
    H, W = LARGE
    u8 = noise((3, H, W, 3), 41)
    C, B, S, Hu, Sh = imgaug.CONTRAST, imgaug.BRIGHTNESS, imgaug.SATURATION, imgaug.HUE, imgaug.SHARPNESS
    masks = np.array([0, C, B, B | C, Sh, C | Sh, S | Hu, 31, Hu, C | S, B | Sh], dtype=np.int32)
    src_index = np.array([2, 2, 0, 1, 1, 0, 2, 0, 1, 2, 2], dtype=np.int32)
    rng = np.random.default_rng(42)
    fac = np.stack([rng.uniform(0.5, 1.5, 11), rng.uniform(0.5, 1.5, 11), rng.uniform(0, 2, 11), rng.uniform(-0.5, 0.5, 11), rng.uniform(0, 2, 11)], axis=1).astype(np.float32)
    oh, ow = 21, 90
    boxes = np.stack([rng.integers(0, W - ow + 1, 11), rng.integers(0, H - oh + 1, 11), rng.integers(0, 2, 11)], axis=1).astype(np.int32)
    for normalise in (True, False):
        both_equal_the_reference(sim, dev, u8, boxes, masks, fac, (oh, ow), src_index, normalise, what="mixed masks")
    # no output has the contrast bit: no reduction at all
    both_equal_the_reference(sim, dev, u8, boxes, masks & ~C, fac, (oh, ow), src_index, True, what="no contrast")


@pytest.mark.parametrize("size", [(5, 67), LARGE, (130, 259)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_sums_behind_contrast(sim, dev, size):
    """S itself through avsim_image_jitter_sums, and through fc = 0, where every pixel of the output is m = float32(S / (N 2^20))."""
    H, W = size
    u8 = noise((3, H, W, 3), 51 + H)
    u8[2] = 255                                                                 # the largest sum an image of this size has
    masks = np.array([2, 3, 2, 3, 2, 3], dtype=np.int32)
    src_index = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
    fac = np.array([[0.8, 0, 1, 0, 1], [1.2, 0, 1, 0, 1], [0, 0, 1, 0, 1], [0.5, 0, 1, 0, 1], [1, 0, 1, 0, 1], [2, 0, 1, 0, 1]], dtype=np.float32)
    boxes = np.zeros((6, 3), dtype=np.int32)
    want = imgaug.gray_sum_reference(u8, imgaug.pack_params(boxes, masks, fac), src_index)
    got = both_equal_the_reference(sim, dev, u8, boxes, masks, fac, (H, W), src_index, False, what="fc = 0")
    m = (want.astype(np.float64) / np.float64(H * W * 1048576)).astype(np.float32)
    assert all((got[i] == m[i]).all() for i in range(6))
    assert np.array_equal(sim.jitter_gray_sums(6), want)
    h, _ = dev
    sums = np.zeros(6, dtype=np.uint64)
    h.check(h.L.avsim_image_jitter_sums(h.h, sums.ctypes.data, 6))
    assert np.array_equal(sums, want)
    assert h.L.avsim_image_jitter_sums(h.h, sums.ctypes.data, 7) == -1


def test_refusals_leave_out_untouched(sim, dev):
    H, W, oh, ow = 7, 9, 4, 5
    u8 = noise((3, H, W, 3), 21)
    t_img = T.from_numpy(u8).to(dev[1])
    L = sim.h.L
    ok = dict(nsrc=3, h=H, w=W, boxes=[(1, 1, 0), (4, 3, 1)], masks=[31, 0], factors=[[1, 1, 1, 0, 1]] * 2, nout=None, src_index=None, out_h=oh, out_w=ow, mean_std=None)

    def arrays(a):
        bm = np.ascontiguousarray(np.concatenate([np.asarray(a["boxes"], dtype=np.int32).reshape(-1, 3), np.asarray(a["masks"], dtype=np.int32).reshape(-1, 1)], axis=1))
        fac = np.ascontiguousarray(a["factors"], dtype=np.float32).reshape(-1, 5)
        si = None if a["src_index"] is None else np.array(a["src_index"], dtype=np.int32)
        ms = None if a["mean_std"] is None else np.array(a["mean_std"], dtype=np.float32)
        return bm, fac, si, ms

    def host(**kw):
        a = dict(ok, **kw)
        bm, fac, si, ms = arrays(a)
        out = np.full((2, 3, oh, ow), 12345.0, dtype=np.float32)
        rc = L.avsim_image_jitter(sim.h.h, u8.ctypes.data, a["nsrc"], a["h"], a["w"], bm.ctypes.data, fac.ctypes.data, _ffi.ptr(si), len(bm) if a["nout"] is None else a["nout"],
                                  _ffi.ptr(ms), a["out_h"], a["out_w"], out.ctypes.data)
        if rc:
            assert (out == np.float32(12345.0)).all(), "a refused call wrote `out`"
            assert rc != -1 or len(L.avsim_last_error(sim.h.h)) > 0
        return rc

    def device(**kw):
        a = dict(ok, **kw)
        bm, fac, si, ms = arrays(a)
        rc, _, intact, untouched = dev_jitter(dev, t_img, (a["nsrc"], a["h"], a["w"]), bm, fac, si, ms, (a["out_h"], a["out_w"]), 1024, a["nout"])
        assert rc == 0 or (untouched and intact), "a refused call wrote `out`"
        assert rc != -1 or len(dev[0].L.avsim_last_error(dev[0].h)) > 0
        return rc

    assert host() == 0 and device() == 0
    assert host(mean_std=[[0.5] * 3, [0.25] * 3], src_index=[2, 0]) == 0
    assert host(masks=[0, 0], factors=[[np.nan, np.inf, -1, 9, 99]] * 2) == 0                      # factors of unset bits are not looked at
    assert host(masks=[31, 31], factors=[[16, 0, 16, 0.5, 16], [0, 16, 0, -0.5, 0]]) == 0           # the ends of the ranges
    nan, inf = float("nan"), float("inf")
    refused = [dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(out_h=0), dict(out_w=0), dict(out_h=65536), dict(out_w=65536),
               dict(nout=0), dict(nout=-1), dict(nsrc=0), dict(nsrc=-1),
               dict(boxes=[(5, 1, 0), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 4, 0)]), dict(boxes=[(-1, 0, 0), (0, 0, 0)]), dict(boxes=[(0, -1, 0), (0, 0, 0)]),
               dict(out_h=8), dict(out_w=10),                                                      # larger than the source
               dict(boxes=[(0, 0, 2), (0, 0, 0)]), dict(boxes=[(0, 0, 0), (0, 0, -1)]), dict(masks=[32, 0]), dict(masks=[0, -1]), dict(masks=[0, 63]),
               dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(nsrc=1),                      # (nsrc = 1: output 1 reads image 1)
               dict(mean_std=[[0.5] * 3, [0.2, 0, 0.2]]), dict(mean_std=[[0.5] * 3, [nan, 0.2, 0.2]]), dict(mean_std=[[0.5] * 3, [0.2, 0.2, inf]])]
    for k in range(5):
        for v in (nan, inf, -inf, (0.50001 if k == 3 else 16.001), (-0.50001 if k == 3 else -0.001)):
            f = [1, 1, 1, 0, 1]
            f[k] = v
            refused.append(dict(masks=[0, 1 << k], factors=[[1, 1, 1, 0, 1], f]))
    for kw in refused:
        assert host(**kw) == -1, kw
        assert device(**kw) == -1, kw
    with pytest.raises(ValueError):
        sim.jitter_images(u8, (np.array([(5, 1, 0, 0)], dtype=np.int32), np.zeros((1, 5), np.float32)), (oh, ow))
    with pytest.raises(ValueError):
        sim.jitter_images(u8, (np.array([(0, 0, 0, 8)], dtype=np.int32), np.array([[1, 1, 1, 0.6, 1]], np.float32)), (oh, ow))


def test_calls_in_a_row_keep_their_own_parameters(dev):
    """Six calls of the same sizes without a synchronisation between them, the caller's arrays overwritten as soon as a call returns: the
    library has copied them (more calls than it has staging slots, so slots are reused behind their events)."""
    h, d = dev
    H, W, oh, ow, n = 33, 130, 20, 64, 5
    u8 = noise((n, H, W, 3), 31)
    t_img = T.from_numpy(u8).to(d)
    rng = np.random.default_rng(32)
    bm, fac, si, ms = np.zeros((n, 4), dtype=np.int32), np.zeros((n, 5), dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros((2, 3), dtype=np.float32)
    outs, wants = [], []
    for k in range(6):
        bm[:, 0], bm[:, 1], bm[:, 2], bm[:, 3] = rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n), rng.integers(0, 32, n)
        fac[:] = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.8, 1.2, n), rng.uniform(0.5, 1.5, n), rng.uniform(-0.05, 0.05, n), rng.uniform(0.8, 1.2, n)], axis=1)
        si[:] = rng.integers(0, n, n)
        ms[0], ms[1] = rng.uniform(0.3, 0.6, 3), rng.uniform(0.2, 0.3, 3)
        wants.append(imgaug.jitter_reference(u8, (bm.copy(), fac.copy()), (oh, ow), ms[0].copy(), ms[1].copy(), si.copy()))
        out = T.empty((n, 3, oh, ow), dtype=T.float32, device=d)
        h.check(h.L.avsim_image_jitter(h.h, t_img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, si.ctypes.data, n, ms.ctypes.data, oh, ow, out.data_ptr()))
        bm[:], fac[:], si[:], ms[:] = 0, 0, 0, 1                              # the caller's arrays are its own again
        outs.append(out)
    T.cuda.synchronize()
    for k in range(6):
        got = outs[k].cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(got, wants[k]), f"call {k}"


def test_the_layers_agree_with_the_reference(sim):
    """VecEnv.jitter_images (tensors, the env's stream) and BatchedSim.jitter_images (numpy) on a small batch, a 2-env insert_peg handle each."""
    from av_aloha_amd.vec_env import make_vec
    H, W, oh, ow = 20, 70, 17, 66
    u8 = noise((2, H, W, 3), 61)
    p = np.zeros(3, dtype=imgaug.PARAMS_DTYPE)
    p["x0"], p["y0"], p["flip"], p["mask"] = [0, 3, 4], [1, 0, 3], [0, 1, 1], [31, 2, 24]
    p["factor"] = [[1.1, 0.9, 1.4, 0.03, 1.2], [1, 1.2, 1, 0, 1], [1, 1, 1, -0.2, 0.5]]
    si = [1, 0, 1]
    want = imgaug.jitter_reference(u8, p, (oh, ow), MEAN, STD, si)
    assert np.array_equal(sim.jitter_images(u8, p, (oh, ow), MEAN, STD, si), want)
    assert np.array_equal(sim.jitter_images(u8, imgaug.split_params(p), (oh, ow), src_index=si), imgaug.jitter_reference(u8, p, (oh, ow), src_index=si))
    env = make_vec("gym_guided_vision/InsertPeg-3Arms-v0", num_envs=2, max_episode_steps=5, cameras=[])
    try:
        t_img = T.from_numpy(u8).to(env.device)
        got = env.jitter_images(t_img, p, (oh, ow), MEAN, STD, si)
        assert got.device == env.device and tuple(got.shape) == (3, 3, oh, ow)
        assert np.array_equal(got.cpu().numpy(), want)
        out = T.empty((3, 3, oh, ow), dtype=T.float32, device=env.device)
        assert env.jitter_images(t_img, p, (oh, ow), src_index=si, out=out) is out
        assert np.array_equal(out.cpu().numpy(), imgaug.jitter_reference(u8, p, (oh, ow), src_index=si))
        with pytest.raises(ValueError):
            env.jitter_images(t_img, p, (oh + 4, ow), MEAN, STD, si)
    finally:
        env.close()
