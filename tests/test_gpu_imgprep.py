"""The device's image statistics and image preparation (avsim_image_stats / avsim_image_prep, csrc/avsim_imgprep.hip.h) against their
specification, av_aloha_amd/imgprep.py: the statistics are integers and the prepared images are table entries, so everything is compared
for equality -- floats as their uint32 bit patterns -- through a host-pointer handle and a device handle.  Shapes: the smallest at which the
kernels can go wrong (image byte counts that are no multiple of 16 or 48 so that image 1 starts unaligned, more rows than a band, the
largest row and column, more samples than a 32-bit sum of squares holds; output widths on both sides of the 16-byte store's condition)."""
import numpy as np
import pytest

from av_aloha_amd import _ffi, imgprep
from avsim_test_util import bits, noise
from gpu_util import Guarded, torch as T
from gpu_util import dev, sim          # noqa: F401  (module-scoped fixtures: this module gets its own handles)

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5 - (1 << 32)      # as an int32


def to_f32(u8_nhwc):
    """u8 [n, H, W, 3] -> float32 [n, 3, H, W] = u8 / 255 (and (int)(v * 255 + 0.5f) gives the u8 back: tests/test_imgprep_host.py)."""
    return np.ascontiguousarray(np.transpose(u8_nhwc, (0, 3, 1, 2)).astype(np.float32) / np.float32(255))


def dev_stats(dev, arr, fmt, index=None, offset=0):
    """avsim_image_stats through the device handle; offset: the images start that many bytes into their allocation."""
    h, d = dev
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = T.zeros(len(raw) + offset + 64, dtype=T.uint8, device=d)
    buf[offset:offset + len(raw)] = T.from_numpy(raw).to(d)
    n, (H, W) = arr.shape[0], (arr.shape[2:] if fmt else arr.shape[1:3])
    t_idx = None if index is None else T.from_numpy(np.asarray(index, dtype=np.int32)).to(d)
    m = n if index is None else len(index)
    out = T.full((m, 3, 4), -1, dtype=T.int64, device=d)
    h.check(h.L.avsim_image_stats(h.h, buf.data_ptr() + offset, fmt, _ffi.ptr(t_idx), m, H, W, out.data_ptr()))
    T.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


# ---- statistics ----------------------------------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (1, 5), (3, 17), (5, 67), (130, 33), (1, 65535), (65535, 1)]


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stats_equal_the_reference(sim, dev, size, fmt):
    H, W = size
    u8 = noise((70, H, W, 3), H * 7 + W)
    want = imgprep.stats_reference(u8)
    for n in (1, 3, 70):
        arr = to_f32(u8[:n]) if fmt else u8[:n]
        got = sim.image_stats(arr)
        assert got.dtype == np.uint64 and np.array_equal(got, want[:n]), f"host mode, {n} images"
        assert np.array_equal(dev_stats(dev, arr, fmt), want[:n]), f"device mode, {n} images"
    # an index with repeats and a reversed order
    index = [2, 2, 0, 1, 2, 0]
    arr = to_f32(u8[:3]) if fmt else u8[:3]
    assert np.array_equal(sim.image_stats(arr, index), want[index])
    assert np.array_equal(dev_stats(dev, arr, fmt, index), want[index])
    # the batch at other distances from a 16-byte boundary
    for offset in ((4, 8, 12) if fmt else (1, 2, 3, 5, 15)):
        assert np.array_equal(dev_stats(dev, arr, fmt, None, offset), want[:3]), f"offset {offset}"


@pytest.mark.parametrize("fmt", [0, 1])
def test_stats_sums_do_not_overflow_32_bits(sim, dev, fmt):
    """300 x 300 of 255: 90 000 samples per channel, a sum of squares of 5.85e9 > 2^32."""
    u8 = np.full((2, 300, 300, 3), 255, dtype=np.uint8)
    want = imgprep.stats_reference(u8)
    assert int(want[0, 0, 1]) == 90000 * 255 * 255 > 2 ** 32
    arr = to_f32(u8) if fmt else u8
    assert np.array_equal(sim.image_stats(arr), want)
    assert np.array_equal(dev_stats(dev, arr, fmt), want)


@pytest.mark.parametrize("fmt", [0, 1])
def test_stats_min_max(sim, dev, fmt):
    zero = np.zeros((2, 9, 21, 3), dtype=np.uint8)
    grey = np.full((3, 37, 53, 3), 128, dtype=np.uint8)
    grey[0, 0, 0, 0], grey[0, 36, 52, 0] = 255, 0            # the first and the last byte positions of a channel
    grey[1, 17, 29, 1], grey[1, 18, 3, 1] = 0, 255
    grey[2, 36, 52, 2], grey[2, 0, 0, 2] = 255, 0
    for u8 in (zero, grey):
        want = imgprep.stats_reference(u8)
        arr = to_f32(u8) if fmt else u8
        assert np.array_equal(sim.image_stats(arr), want)
        assert np.array_equal(dev_stats(dev, arr, fmt), want)
    assert imgprep.stats_reference(grey)[1, 1, 2:].tolist() == [0, 255] and imgprep.stats_reference(grey)[1, 0, 2:].tolist() == [128, 128]


def test_stats_refusals_leave_out_untouched(sim, dev):
    u8 = noise((2, 4, 6, 3), 9)
    L = sim.h.L
    out = np.full((2, 3, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    keep = out.copy()
    for fmt, n, H, W in ((2, 2, 4, 6), (-1, 2, 4, 6), (0, 0, 4, 6), (0, -1, 4, 6), (0, 2, 0, 6), (0, 2, 4, 0), (0, 1, 65536, 1), (0, 1, 1, 65536)):
        assert L.avsim_image_stats(sim.h.h, u8.ctypes.data, fmt, None, n, H, W, out.ctypes.data) == -1, (fmt, n, H, W)
        assert np.array_equal(out, keep)
    bad = np.array([0, -1], dtype=np.int32)
    assert L.avsim_image_stats(sim.h.h, u8.ctypes.data, 0, bad.ctypes.data, 2, 4, 6, out.ctypes.data) == -1 and np.array_equal(out, keep)
    with pytest.raises(ValueError):
        sim.image_stats(u8, [0, 2])
    h, d = dev
    t_img, t_out = T.from_numpy(u8).to(d), T.full((2, 3, 4), 77, dtype=T.int64, device=d)
    for fmt, n, H, W in ((2, 2, 4, 6), (0, 0, 4, 6), (0, 2, 0, 6), (0, 2, 4, 65536)):
        assert h.L.avsim_image_stats(h.h, t_img.data_ptr(), fmt, None, n, H, W, t_out.data_ptr()) == -1
    T.cuda.synchronize()
    assert (t_out == 77).all().item()


# ---- preparation ---------------------------------------------------------------------------------------------------------------------------

def tables():
    """Three tables with distinctive values: a normalisation, one that holds -0.0 and inf, one of random bit patterns' floats."""
    rng = np.random.default_rng(11)
    t0 = imgprep.normalise_lut([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    t1 = rng.standard_normal((3, 256)).astype(np.float32)
    t1[:, ::7] = np.float32(-0.0)
    t1[:, 3::11] = np.float32(np.inf)
    t1[1, 5::13] = np.float32(-np.inf)
    t2 = (np.arange(768, dtype=np.float32).reshape(3, 256) * np.float32(-1.5) + np.float32(1e-3)).astype(np.float32)
    return np.ascontiguousarray(np.stack([t0, t1, t2]), dtype=np.float32)


def boxes_for(H, W, oh, ow, n):
    """n boxes that touch every border, with odd and even x0, flips mixed."""
    xs = sorted({0, W - ow, min(1, W - ow), min(2, W - ow), (W - ow) // 2, max(0, W - ow - 1)})
    ys = sorted({0, H - oh, (H - oh) // 2})
    return np.array([(xs[i % len(xs)], ys[(i // 2) % len(ys)], (i + i // 3) % 2) for i in range(n)], dtype=np.int32)


def dev_prep(dev, arr, fmt, lut, lut_index, box, src_index, out_hw, guard):
    """avsim_image_prep through the device handle into the middle of a sentinel-filled tensor -> (rc, out, no word before or after it was
    written, none of it was written)."""
    h, d = dev
    n, (H, W) = arr.shape[0], (arr.shape[2:] if fmt else arr.shape[1:3])
    oh, ow = out_hw
    g = Guarded(d, len(box) * 3 * oh * ow, T.int32, SENTINEL, guard, 1024)
    t_img, t_lut = T.from_numpy(np.ascontiguousarray(arr)).to(d), T.from_numpy(lut).to(d)
    li = None if lut_index is None else np.ascontiguousarray(lut_index, dtype=np.int32)
    si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32)
    b = np.ascontiguousarray(box, dtype=np.int32)
    rc = h.L.avsim_image_prep(h.h, t_img.data_ptr(), fmt, n, H, W, t_lut.data_ptr(), len(lut), _ffi.ptr(li), b.ctypes.data, len(b), _ffi.ptr(si), oh, ow,
                              g.ptr())
    T.cuda.synchronize()
    out, intact, untouched = g.read()
    return rc, out.view(np.uint32).reshape(len(box), 3, oh, ow), intact, untouched


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("size", [(7, 9), (33, 130), (48, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_prep_equals_the_reference(sim, dev, size, fmt):
    H, W = size
    u8 = noise((3, H, W, 3), H + W)
    arr = to_f32(u8) if fmt else u8
    lut = tables()
    case = 0
    for ow in (1, 3, 4, 5, 64, 129, W):
        if ow > W:
            continue
        for oh in (1, H):
            n = 7
            box = boxes_for(H, W, oh, ow, n)
            src_index = np.array([2, 0, 0, 1, 2, 2, 1], dtype=np.int32)       # repeats
            lut_index = np.array([0, 1, 2, 2, 1, 0, 1], dtype=np.int32)
            want = bits(imgprep.prep_reference(u8, lut, lut_index, box, (oh, ow), src_index))
            guard = 1024 if case % 2 == 0 else 1021                            # `out` on and off a 16-byte boundary
            case += 1
            rc, got, intact, _ = dev_prep(dev, arr, fmt, lut, lut_index, box, src_index, (oh, ow), guard)
            assert rc == 0 and np.array_equal(got, want), f"device mode, {oh} x {ow}"
            assert intact, f"device mode, {oh} x {ow}: bytes outside `out` were written"
            assert np.array_equal(bits(sim.prep_images(arr, lut, box, (oh, ow), lut_index, src_index)), want), f"host mode, {oh} x {ow}"
    # the full-image box, NULL index arrays: output i reads image i through table 0
    box = np.array([(0, 0, 0), (0, 0, 1), (0, 0, 0)], dtype=np.int32)
    want = bits(imgprep.prep_reference(u8, lut, None, box, (H, W)))
    rc, got, intact, _ = dev_prep(dev, arr, fmt, lut, None, box, None, (H, W), 1022)
    assert rc == 0 and np.array_equal(got, want) and intact
    assert np.array_equal(bits(sim.prep_images(arr, lut, box, (H, W))), want)


def test_prep_refusals_leave_out_untouched(sim, dev):
    H, W, oh, ow = 7, 9, 4, 5
    u8 = noise((3, H, W, 3), 21)
    lut = tables()
    ok_box = np.array([(1, 1, 0), (4, 3, 1)], dtype=np.int32)
    L = sim.h.L

    def host(fmt=0, nsrc=3, h=H, w=W, nlut=3, lut_index=None, box=ok_box, nout=None, src_index=None, out_h=oh, out_w=ow):
        out = np.full((2, 3, oh, ow), 12345.0, dtype=np.float32)
        li = None if lut_index is None else np.array(lut_index, dtype=np.int32)
        si = None if src_index is None else np.array(src_index, dtype=np.int32)
        b = np.ascontiguousarray(box, dtype=np.int32)
        rc = L.avsim_image_prep(sim.h.h, u8.ctypes.data, fmt, nsrc, h, w, lut.ctypes.data, nlut, _ffi.ptr(li), b.ctypes.data, len(b) if nout is None else nout,
                                _ffi.ptr(si), out_h, out_w, out.ctypes.data)
        assert (out == np.float32(12345.0)).all() or rc == 0, "a refused call wrote `out`"
        return rc

    assert host() == 0
    refused = [dict(fmt=2), dict(fmt=-1), dict(h=0), dict(w=0), dict(h=65536), dict(w=65536), dict(out_h=0), dict(out_w=0), dict(out_h=65536),
               dict(out_w=65536), dict(nout=0), dict(nout=-1), dict(nsrc=0), dict(nlut=0),
               dict(box=[(5, 1, 0), (0, 0, 0)]), dict(box=[(0, 0, 0), (0, 4, 0)]), dict(box=[(-1, 0, 0), (0, 0, 0)]), dict(box=[(0, -1, 0), (0, 0, 0)]),
               dict(out_h=8), dict(out_w=10),                                    # larger than the source
               dict(box=[(0, 0, 2), (0, 0, 0)]), dict(box=[(0, 0, 0), (0, 0, -1)]),
               dict(lut_index=[0, 3]), dict(lut_index=[-1, 0]), dict(src_index=[3, 0]), dict(src_index=[0, -1]), dict(nsrc=1)]      # (nsrc = 1: output 1 reads image 1)
    for kw in refused:
        assert host(**kw) == -1, kw
    with pytest.raises(ValueError):
        sim.prep_images(u8, lut, [(5, 1, 0)], (oh, ow))
    # the device handle: the same checks run on the host arrays before anything is launched
    for kw in (dict(box=[(5, 1, 0), (0, 0, 0)]), dict(box=[(0, 0, 2), (0, 0, 0)]), dict(lut_index=[0, 3]), dict(src_index=[3, 0])):
        rc, _, intact, untouched = dev_prep(dev, u8, 0, lut, kw.get("lut_index"), kw.get("box", ok_box), kw.get("src_index"), (oh, ow), 1024)
        assert rc == -1 and untouched and intact, kw
    h, d = dev
    t_img, t_lut, t_out = T.from_numpy(u8).to(d), T.from_numpy(lut).to(d), T.full((2, 3, oh, ow), 7.0, device=d)
    for fmt, oh_, ow_ in ((2, oh, ow), (0, 0, ow), (0, oh, 65536)):
        assert h.L.avsim_image_prep(h.h, t_img.data_ptr(), fmt, 3, H, W, t_lut.data_ptr(), 3, None, ok_box.ctypes.data, 2, None, oh_, ow_, t_out.data_ptr()) == -1
    T.cuda.synchronize()
    assert (t_out == 7.0).all().item()


def test_prep_through_both_fronts(sim):
    """BatchedSim.prep_images (numpy) and VecEnv.prep_images (torch) are one body behind two kinds of array: the same bytes from both, with
    the table and source index arrays given, and those of the specification.  An output width of 6: rows that the 16-byte store cannot take."""
    from av_aloha_amd.vec_env import make_vec
    u8, lut, out_hw = noise((2, 9, 11, 3), 41), tables(), (4, 6)
    box, lut_index, src_index = [(0, 0, 0), (5, 5, 1), (2, 3, 0)], [0, 2, 1], [1, 0, 1]
    want = bits(imgprep.prep_reference(u8, lut, lut_index, box, out_hw, src_index))
    env = make_vec("gym_guided_vision/InsertPeg-3Arms-v0", num_envs=2, max_episode_steps=5, cameras=[])
    try:
        t_lut = T.from_numpy(lut).to(env.device)
        for arr in (u8, to_f32(u8)):
            a = sim.prep_images(arr, lut, box, out_hw, lut_index, src_index)
            t = env.prep_images(T.from_numpy(arr).to(env.device), t_lut, box, out_hw, lut_index, src_index)
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and t.dtype == T.float32 and t.device == env.device
            assert a.shape == tuple(t.shape) == (3, 3, 4, 6)
            assert a.tobytes() == t.cpu().numpy().tobytes() == want.tobytes()
    finally:
        env.close()


def test_prep_calls_in_a_row_keep_their_own_boxes(dev):
    """Six calls without a synchronisation between them, the caller's arrays overwritten as soon as a call returns: the library has copied
    them (more calls than it has staging slots, so slots are reused behind their events)."""
    h, d = dev
    H, W, oh, ow, n = 33, 130, 20, 64, 5
    u8 = noise((n, H, W, 3), 31)
    lut = tables()
    t_img, t_lut = T.from_numpy(u8).to(d), T.from_numpy(lut).to(d)
    rng = np.random.default_rng(32)
    box, li, si = np.zeros((n, 3), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    outs, wants = [], []
    for k in range(6):
        box[:, 0], box[:, 1], box[:, 2] = rng.integers(0, W - ow + 1, n), rng.integers(0, H - oh + 1, n), rng.integers(0, 2, n)
        li[:], si[:] = rng.integers(0, 3, n), rng.integers(0, n, n)
        wants.append(bits(imgprep.prep_reference(u8, lut, li, box, (oh, ow), si)))
        out = T.empty((n, 3, oh, ow), dtype=T.float32, device=d)
        h.check(h.L.avsim_image_prep(h.h, t_img.data_ptr(), 0, n, H, W, t_lut.data_ptr(), 3, li.ctypes.data, box.ctypes.data, n, si.ctypes.data, oh, ow,
                                     out.data_ptr()))
        box[:], li[:], si[:] = 0, 0, 0                       # the caller's arrays are its own again
        outs.append(out)
    T.cuda.synchronize()
    for k in range(6):
        assert np.array_equal(bits(outs[k].cpu().numpy()), wants[k]), f"call {k}"
