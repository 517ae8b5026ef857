"""The device's image resize (avsim_image_resize, csrc/avsim_imgresize.hip: k_resize<class, format>) against its specification,
av_aloha_amd/imgresize.py (resize_reference).  Every comparison is np.array_equal on the float32 arrays with no NaN in either -- equality of
bits, -0 and +0 aside -- through a host-pointer handle and a device handle, for both formats and both antialias settings.  Inputs: noise with
fixed seeds; u8 images for format 0, normal floats (values outside [0, 1] too: the format is read as floats) for format 1; nsrc = 3, so
images 1 and 2 start off a 4-byte boundary wherever 3 H W % 4 != 0.  The kernels' tiles are 16 x 64 (ratio <= 2), 8 x 32 (<= 5) and 4 x 32
(<= 16) output pixels, and the shapes are the smallest that give several tiles each way in each class."""
import numpy as np
import pytest

from av_aloha_amd import _ffi, imgaug, imgresize
from gpu_util import Guarded, torch as T
from gpu_util import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5 - (1 << 32)      # as an int32
MEAN, STD, FILL = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225], [0.25, -0.5, 0.75]


def source(fmt, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if fmt == 0:
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    return rng.standard_normal((n, 3, H, W)).astype(np.float32)


def shape_of(img, fmt):
    return (img.shape[0], img.shape[1], img.shape[2]) if fmt == 0 else (img.shape[0], img.shape[2], img.shape[3])


def arrays(sb, dst, si, fill, ms):
    sb = np.ascontiguousarray(sb, dtype=np.int32).reshape(-1, 5)
    dst = np.ascontiguousarray(dst, dtype=np.int32).reshape(-1, 4)
    si = None if si is None else np.ascontiguousarray(si, dtype=np.int32)
    fill = None if fill is None else np.ascontiguousarray(fill, dtype=np.float32)
    ms = None if ms is None else np.ascontiguousarray(ms, dtype=np.float32)
    return sb, dst, si, fill, ms


def dev_resize(dev, t_img, fmt, shape, sb, dst, si, aa, fill, ms, out_hw, guard, nout=None):
    """avsim_image_resize through the device handle into the middle of a sentinel-filled tensor -> (rc, out, no word around it was
    written, none of it was written)."""
    h, d = dev
    n, H, W = shape
    oh, ow = out_hw
    size = len(sb) * 3 * oh * ow if 0 < oh < 65536 and 0 < ow < 65536 else 64
    g = Guarded(d, size, T.int32, SENTINEL, guard, 1024)
    rc = h.L.avsim_image_resize(h.h, t_img.data_ptr(), fmt, n, H, W, sb.ctypes.data, dst.ctypes.data, _ffi.ptr(si), len(sb) if nout is None else nout, aa, _ffi.ptr(fill),
                                _ffi.ptr(ms), oh, ow, g.ptr())
    T.cuda.synchronize()
    out, intact, untouched = g.read()
    return rc, out.view(np.uint32), intact, untouched


_case = [0]


def both_equal_the_reference(sim, dev, img, fmt, sb, dst, out_hw, aa, fill=None, mean=None, std=None, si=None, what="", want=None):
    """One call through each handle against imgresize.resize_reference (want: the reference, where the caller has it already)."""
    if want is None:
        want = imgresize.resize_reference(img, fmt, sb, dst, out_hw, aa, fill, mean, std, si)
    assert want.dtype == np.float32 and not np.isnan(want).any()
    got = sim.resize_images(img, sb, dst, out_hw, aa, fill, mean, std, si)
    assert got.dtype == np.float32 and not np.isnan(got).any() and np.array_equal(got, want), f"host mode: {what}"
    guard = 1024 if _case[0] % 2 == 0 else 1021                                # `out` on and off a 16-byte boundary
    _case[0] += 1
    a = arrays(sb, dst, si, fill, imgresize.mean_std(mean, std))
    rc, out, intact, _ = dev_resize(dev, T.from_numpy(img).to(dev[1]), fmt, shape_of(img, fmt), a[0], a[1], a[2], aa, a[3], a[4], out_hw, guard)
    out = out.view(np.float32).reshape(want.shape)
    assert rc == 0 and not np.isnan(out).any() and np.array_equal(out, want), f"device mode: {what}"
    assert intact, f"device mode: {what}: bytes outside `out` were written"
    return got


# (source H x W, output h x w): neither a tile multiple; a non-integer ratio > 2 whose taps straddle tiles; an upscale; the ratio cap; and per
# class a shape of several tiles each way (ratios 1.3, 2.3 and 10.7 / 10)
SHAPES = [((37, 53), (20, 17)), ((48, 64), (17, 23)), ((30, 40), (45, 61)), ((64, 64), (4, 4)), ((46, 133), (35, 100)), ((41, 300), (18, 130)), ((96, 700), (9, 70))]


@pytest.mark.parametrize("aa", [1, 0], ids=["antialias", "plain"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["u8", "float"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_whole_images(sim, dev, shape, fmt, aa):
    """The whole image to the whole output, plain and mirrored, from the sources in turn, with and without fill / mean / std."""
    (H, W), (oh, ow) = shape
    img = source(fmt, 3, H, W, 7 * H + W)
    sb = [(0, 0, W, H, 0), (0, 0, W, H, 1), (0, 0, W, H, 0)]
    dst = [(0, 0, ow, oh)] * 3
    both_equal_the_reference(sim, dev, img, fmt, sb, dst, (oh, ow), aa, None, None, None, [2, 1, 0], what=f"{shape}")
    got = both_equal_the_reference(sim, dev, img, fmt, sb, dst, (oh, ow), aa, FILL, MEAN, STD, None, what=f"{shape} normalised")
    assert got.shape == (3, 3, oh, ow)


@pytest.mark.parametrize("aa", [1, 0], ids=["antialias", "plain"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["u8", "float"])
def test_boxes_rectangles_and_classes_in_one_call(sim, dev, fmt, aa):
    """Eight outputs with eight different boxes: on each of the four borders, the whole image, strictly inside, a 1 x 1 box and a box at the
    ratio cap; mirrored and not; rectangles padded on the left and on top, on the right and below, on all sides and not at all; a 1 x 1
    rectangle; sources repeated; all three ratio classes; a fill that is not 0, with and without mean / std."""
    H, W, oh, ow = 50, 135, 21, 70
    img = source(fmt, 3, H, W, 11)
    sb = [(0, 0, 60, 30, 0), (W - 97, 0, 97, 41, 1), (0, H - 33, 101, 33, 1), (W - 135, H - 50, 135, 50, 0), (3, 2, 129, 47, 1), (77, 31, 1, 1, 0), (0, 0, 128, 48, 0),
          (5, 5, 16, 16, 1)]
    dst = [(ow - 60, oh - 20, 60, 20), (0, 0, 40, 17), (3, 2, 64, 18), (0, 0, ow, oh), (1, 1, 33, 9), (65, 20, 5, 1), (31, 9, 8, 3), (69, 0, 1, 1)]
    si = [0, 1, 2, 2, 1, 1, 0, 2]
    classes = [imgresize.resize_taps(b[2], d[2], 1)[2].shape[1] for b, d in zip(sb, dst)]
    assert min(classes) <= 5 and any(5 < k <= 11 for k in classes) and max(classes) == 33
    both_equal_the_reference(sim, dev, img, fmt, sb, dst, (oh, ow), aa, FILL, MEAN, STD, si, what="eight boxes")
    got = both_equal_the_reference(sim, dev, img, fmt, sb, dst, (oh, ow), aa, FILL, None, None, si, what="eight boxes, no mean / std")
    assert (got[5, :, :20] == np.array(FILL, dtype=np.float32).reshape(3, 1, 1)).all()
    both_equal_the_reference(sim, dev, img, fmt, sb[:3], dst[:3], (oh, ow), aa, None, None, None, None, what="no src_index, no fill")


@pytest.mark.parametrize("fmt", [0, 1], ids=["u8", "float"])
def test_one_by_one(sim, dev, fmt):
    """A 1 x 1 output from a 1 x 1 box, from a 16 x 16 box and from a 1 x 16 box; a 1 x 1 image; a 1 x 1 box blown up."""
    img = source(fmt, 3, 16, 19, 13)
    for aa in (0, 1):
        both_equal_the_reference(sim, dev, img, fmt, [(18, 15, 1, 1, 0), (3, 0, 16, 16, 1), (0, 7, 16, 1, 0)], [(0, 0, 1, 1)] * 3, (1, 1), aa, FILL, MEAN, STD, what="1 x 1 output")
        both_equal_the_reference(sim, dev, img, fmt, [(0, 0, 1, 1, 0), (18, 15, 1, 1, 1)], [(1, 0, 5, 7), (0, 0, 6, 7)], (7, 6), aa, FILL, what="1 x 1 box blown up")
        one = source(fmt, 2, 1, 1, 14)
        both_equal_the_reference(sim, dev, one, fmt, [(0, 0, 1, 1, 0)] * 2, [(0, 0, 1, 1), (2, 1, 1, 1)], (3, 3), aa, None, None, None, [1, 0], what="1 x 1 image")


def test_more_outputs_than_one_grid_chunk(sim, dev):
    """65541 outputs of 1 x 2 pixels from three small images: the launch goes in chunks of 65535 outputs.  The reference of the eight
    distinct outputs, repeated."""
    img = source(0, 3, 9, 11, 17)
    n = 65541
    sb8 = np.array([(0, 0, 11, 9, 0), (1, 1, 4, 4, 1), (7, 5, 4, 4, 0), (0, 0, 1, 1, 0), (2, 0, 9, 9, 1), (0, 3, 11, 2, 0), (5, 5, 6, 4, 1), (10, 8, 1, 1, 0)], dtype=np.int32)
    dst8 = np.array([(0, 0, 2, 1), (0, 0, 1, 1), (1, 0, 1, 1), (0, 0, 2, 1), (0, 0, 2, 1), (1, 0, 1, 1), (0, 0, 2, 1), (0, 0, 1, 1)], dtype=np.int32)
    si8 = np.array([0, 1, 2, 2, 1, 0, 2, 1], dtype=np.int32)
    want8 = imgresize.resize_reference(img, 0, sb8, dst8, (1, 2), 1, FILL, MEAN, STD, si8)
    k = np.arange(n) % 8
    both_equal_the_reference(sim, dev, img, 0, sb8[k], dst8[k], (1, 2), 1, FILL, MEAN, STD, si8[k], what="65541 outputs", want=np.ascontiguousarray(want8[k]))


def test_refusals_leave_out_untouched(sim, dev):
    H, W, oh, ow = 64, 80, 16, 20
    u8 = source(0, 3, H, W, 21)
    t_img = T.from_numpy(u8).to(dev[1])
    L = sim.h.L
    ok = dict(fmt=0, nsrc=3, h=H, w=W, src_box=[(0, 0, 80, 64, 0), (8, 8, 64, 48, 1)], dst=[(0, 0, 20, 16), (2, 3, 10, 8)], src_index=None, nout=None, aa=1, fill=None,
              mean_std=None, out_h=oh, out_w=ow)

    def reference(a):
        ms = a["mean_std"]
        return imgresize.resize_reference(u8, 0, a["src_box"], a["dst"], (oh, ow), a["aa"], a["fill"], *((ms[0], ms[1]) if ms is not None else (None, None)), a["src_index"])

    def host(**kw):
        a = dict(ok, **kw)
        sb, dst, si, fill, ms = arrays(a["src_box"], a["dst"], a["src_index"], a["fill"], a["mean_std"])
        out = np.full((2, 3, oh, ow), 12345.0, dtype=np.float32)
        rc = L.avsim_image_resize(sim.h.h, u8.ctypes.data, a["fmt"], a["nsrc"], a["h"], a["w"], sb.ctypes.data, dst.ctypes.data, _ffi.ptr(si), len(sb) if a["nout"] is None else a["nout"],
                                  a["aa"], _ffi.ptr(fill), _ffi.ptr(ms), a["out_h"], a["out_w"], out.ctypes.data)
        if rc:
            assert (out == np.float32(12345.0)).all(), "a refused call wrote `out`"
            assert rc != -1 or len(L.avsim_last_error(sim.h.h)) > 0
        else:
            assert np.array_equal(out, reference(a))
        return rc

    def device(**kw):
        a = dict(ok, **kw)
        sb, dst, si, fill, ms = arrays(a["src_box"], a["dst"], a["src_index"], a["fill"], a["mean_std"])
        rc, out, intact, untouched = dev_resize(dev, t_img, a["fmt"], (a["nsrc"], a["h"], a["w"]), sb, dst, si, a["aa"], fill, ms, (a["out_h"], a["out_w"]), 1024, a["nout"])
        assert intact
        assert untouched if rc else np.array_equal(out.view(np.float32).reshape(2, 3, oh, ow), reference(a)), "a refused call wrote `out`"
        assert rc != -1 or len(dev[0].L.avsim_last_error(dev[0].h)) > 0
        return rc

    nan, inf = float("nan"), float("inf")
    full = (0, 0, 80, 64, 0)
    assert host() == 0 and device() == 0
    assert host(mean_std=[[0.5] * 3, [0.25] * 3], src_index=[2, 0], aa=0, fill=[0.1, 0.2, 0.3]) == 0
    assert host(dst=[(0, 0, 5, 4), (0, 0, 20, 16)], src_box=[full, full]) == 0 and device(dst=[(0, 0, 5, 4), (0, 0, 20, 16)], src_box=[full, full]) == 0          # 16 : 1 itself
    refused = [dict(fmt=2), dict(fmt=-1), dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(out_h=0), dict(out_w=0), dict(out_h=65536), dict(out_w=65536),
               dict(nout=0), dict(nout=-1), dict(nsrc=0), dict(nsrc=-1),
               dict(src_box=[(0, 0, 81, 64, 0), full]), dict(src_box=[(0, 1, 80, 64, 0), full]), dict(src_box=[(-1, 0, 80, 64, 0), full]), dict(src_box=[full, (0, -1, 80, 64, 0)]),
               dict(h=63), dict(w=79),
               dict(dst=[(1, 0, 20, 16), (0, 0, 20, 16)]), dict(dst=[(0, 1, 20, 16), (0, 0, 20, 16)]), dict(dst=[(-1, 0, 20, 16), (0, 0, 20, 16)]), dict(dst=[(0, 0, 20, 16), (0, -1, 20, 15)]),
               dict(out_h=15), dict(out_w=19),
               dict(src_box=[(0, 0, 0, 64, 0), full]), dict(src_box=[(0, 0, 80, 0, 0), full]), dict(src_box=[(0, 0, -3, 64, 0), full]), dict(src_box=[full, (0, 0, 80, -1, 0)]),
               dict(dst=[(0, 0, 0, 16), (0, 0, 20, 16)]), dict(dst=[(0, 0, 20, 0), (0, 0, 20, 16)]), dict(dst=[(0, 0, 20, 16), (0, 0, -2, 16)]),
               dict(src_box=[full, full], dst=[(0, 0, 4, 16), (0, 0, 20, 16)]), dict(src_box=[full, full], dst=[(0, 0, 20, 16), (0, 0, 20, 3)]),          # 20 : 1 and 21.3 : 1
               dict(src_box=[(0, 0, 80, 64, 2), full]), dict(src_box=[full, (0, 0, 80, 64, -1)]), dict(aa=2), dict(aa=-1),
               dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(nsrc=1),
               dict(fill=[0, nan, 0]), dict(fill=[inf, 0, 0]), dict(fill=[0, 0, -inf]),
               dict(mean_std=[[0.5] * 3, [0.2, 0, 0.2]]), dict(mean_std=[[0.5] * 3, [nan, 0.2, 0.2]]), dict(mean_std=[[0.5] * 3, [0.2, 0.2, inf]])]
    for kw in refused:
        assert host(**kw) == -1, kw
        assert device(**kw) == -1, kw
    assert host() == 0 and device() == 0                                      # and the handles still compute the specification
    # 16.1 : 1 (161 rows -> 10), refused; 160 -> 10 is not
    tall = source(0, 1, 161, 20, 22)
    with pytest.raises(ValueError):
        sim.resize_images(tall, [(0, 0, 20, 161, 0)], [(0, 0, 20, 10)], (10, 20))
    both_equal_the_reference(sim, dev, tall, 0, [(0, 1, 20, 160, 0)], [(0, 0, 20, 10)], (10, 20), 1, what="160 -> 10")
    with pytest.raises(ValueError):
        sim.resize_images(u8, [full], [(0, 0, 20, 16)], (16, 20), antialias=3)


def test_calls_in_a_row_do_not_wait(dev):
    """Six calls of the same sizes without a synchronisation between them, the caller's arrays overwritten as soon as a call returns (more
    calls than staging slots): the library has copied them, and the stream alone orders the copies and the kernels."""
    h, d = dev
    H, W, oh, ow, n = 33, 130, 20, 64, 9
    u8 = source(0, n, H, W, 31)
    t_img = T.from_numpy(u8).to(d)
    rng = np.random.default_rng(32)
    sb, dst, si, fill, ms = np.zeros((n, 5), dtype=np.int32), np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(3, dtype=np.float32), np.zeros((2, 3), dtype=np.float32)
    outs, wants = [], []
    for k in range(6):
        sb[:, 2], sb[:, 3] = rng.integers(20, W + 1, n), rng.integers(10, H + 1, n)
        sb[:, 0], sb[:, 1], sb[:, 4] = rng.integers(0, W - sb[:, 2] + 1), rng.integers(0, H - sb[:, 3] + 1), rng.integers(0, 2, n)
        dst[:, 2], dst[:, 3] = rng.integers(10, ow + 1, n), rng.integers(5, oh + 1, n)
        dst[:, 0], dst[:, 1] = rng.integers(0, ow - dst[:, 2] + 1), rng.integers(0, oh - dst[:, 3] + 1)
        si[:] = rng.integers(0, n, n)
        fill[:] = rng.uniform(0, 1, 3)
        ms[0], ms[1] = rng.uniform(0.3, 0.6, 3), rng.uniform(0.2, 0.3, 3)
        wants.append(imgresize.resize_reference(u8, 0, sb.copy(), dst.copy(), (oh, ow), k % 2, fill.copy(), ms[0].copy(), ms[1].copy(), si.copy()))
        out = T.empty((n, 3, oh, ow), dtype=T.float32, device=d)
        h.check(h.L.avsim_image_resize(h.h, t_img.data_ptr(), 0, n, H, W, sb.ctypes.data, dst.ctypes.data, si.ctypes.data, n, k % 2, fill.ctypes.data, ms.ctypes.data, oh, ow,
                                       out.data_ptr()))
        sb[:], dst[:], si[:], fill[:], ms[:] = 0, 0, 0, 7, 1                  # the caller's arrays are its own again
        outs.append(out)
    T.cuda.synchronize()
    for k in range(6):
        got = outs[k].cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(got, wants[k]), f"call {k}"


def test_the_layers_agree_with_the_reference(sim):
    """DeviceImages.resize_images (tensors, torch's stream) on u8 frames and on a jitter_images result (float, not quantised), and
    BatchedSim.resize_images (numpy), with a letterbox plan."""
    from av_aloha_amd.images import DeviceImages
    H, W, oh, ow = 24, 70, 16, 32
    u8 = source(0, 2, H, W, 61)
    plan = imgresize.resize_with_pad_plan((H, W), (oh, ow))
    assert plan == (0, 6, 32, 10)
    sb, dst = imgresize.boxes([(0, 0, 0), (0, 0, 1), (0, 0, 0)], (H, W), (oh, ow), "pad")
    assert [tuple(r) for r in dst] == [plan] * 3
    si = [1, 0, 1]
    want = imgresize.resize_reference(u8, 0, sb, dst, (oh, ow), 1, None, MEAN, STD, si)
    assert np.array_equal(sim.resize_images(u8, sb, dst, (oh, ow), True, None, MEAN, STD, si), want)
    di = DeviceImages()
    try:
        t_img = T.from_numpy(u8).to(di.device)
        got = di.resize_images(t_img, sb, dst, (oh, ow), mean=MEAN, std=STD, src_index=si)
        assert got.device == di.device and tuple(got.shape) == (3, 3, oh, ow) and np.array_equal(got.cpu().numpy(), want)
        out = T.empty((3, 3, oh, ow), dtype=T.float32, device=di.device)
        assert di.resize_images(t_img, sb, dst, (oh, ow), antialias=False, fill=FILL, src_index=si, out=out) is out
        assert np.array_equal(out.cpu().numpy(), imgresize.resize_reference(u8, 0, sb, dst, (oh, ow), 0, FILL, src_index=si))
        # a jitter output, in [0, 1] and not on the u8 grid, resized as floats
        p = np.zeros(2, dtype=imgaug.PARAMS_DTYPE)
        p["x0"], p["y0"], p["mask"] = [2, 0], [1, 3], [7, 5]
        p["factor"] = [[1.1, 0.9, 1.4, 0, 1], [0.9, 1, 0.7, 0, 1]]
        crop = (20, 66)
        jit = di.jitter_images(t_img, p, crop)
        want_jit = imgaug.jitter_reference(u8, p, crop)
        sb2, dst2 = imgresize.boxes(np.zeros((2, 3), dtype=np.int32), crop, (oh, ow), "stretch")
        got = di.resize_images(jit, sb2, dst2, (oh, ow), mean=MEAN, std=STD)
        assert np.array_equal(got.cpu().numpy(), imgresize.resize_reference(want_jit, 1, sb2, dst2, (oh, ow), 1, None, MEAN, STD))
        with pytest.raises(ValueError):
            di.resize_images(t_img, [(0, 0, W + 1, H, 0)], [(0, 0, ow, oh)], (oh, ow))
    finally:
        di.close()
