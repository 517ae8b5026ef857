"""Resizing images on the device: the specification of avsim_image_resize (csrc/avsim_imgresize.hip) in numpy, bit for bit (-0 / +0 aside).

The filter is the separable triangle filter of torch's interpolate(mode="bilinear", align_corners=False, antialias=...): with antialias and a
ratio n_in / n_out >= 1 the triangle is as wide as the ratio, otherwise it is the two-tap bilinear kernel.  Every operation below is a float32
operation rounded on its own -- no fused multiply-add --, and the device performs the same ones in the same order.

* `resize_taps(n_in, n_out, antialias)` -> (lo int32 [n_out], count int32 [n_out], weight float32 [n_out, K]): output index i reads the inputs
  lo[i] .. lo[i] + count[i] - 1 with weight[i, :count[i]] (the rest of the row is 0).  In float32:
      scale = f32(n_in) / f32(n_out);  support = scale, inv = 1 / scale when antialias and scale >= 1, else support = 1, inv = 1
      center = scale * (f32(i) + 0.5)
      lo = max(0, int((center - support) + 0.5)), hi = min(n_in, int((center + support) + 0.5))          (int() truncates)
      raw[j] = max(0, 1 - |((f32(j) - center) + 0.5) * inv|) for j in [lo, hi);  tot = the raw weights added in ascending j
      weight = raw / tot;  K = 2 ceil(support) + 1
* `resize_reference(img, fmt, src_box, dst, out_hw, antialias, fill, mean, std, src_index)`: output i reads image src_index[i] (None: i);
  fmt 0 is u8 [n, H, W, 3] with value f32(u) / f32(255), fmt 1 is float32 [n, 3, H, W] read as floats (not quantised, so that a jitter output
  resizes without a loss).  src_box[i] = (x0, y0, w, h, flip) is the source region: the taps are those of a w x h image, so a crop followed
  by a resize equals resizing the cropped image and no pixel outside the box is read.  dst[i] = (ox, oy, rw, rh) is the rectangle of the
  out_h x out_w output the resized region fills; every other pixel is fill[c].  The horizontal pass (h x w -> h x rw) comes first, then the
  vertical one (-> rh x rw); a pass is acc = 0; acc = acc + v[k] * weight[k] over the `count` taps in ascending k, the product and the sum
  rounded separately.  flip mirrors the resized rectangle (x -> rw - 1 - x).  Last, every output pixel, fill included, becomes
  (v - mean[c]) / std[c] (mean / std None: it stays).
* `resize_with_pad_plan(src_hw, out_hw, side)`: the rectangle of the VLA policies' resize_with_pad -- the aspect ratio kept, the padding on
  the left and on top ("top_left") or split evenly ("center").
* `check_resize`: the conditions avsim_image_resize puts on its arguments (include/avsim.h); raises ValueError."""
import functools

import numpy as np

MAX_RATIO = 16            # the largest n_in / n_out per axis (K <= 33)
_F = np.float32


@functools.lru_cache(maxsize=256)
def _taps(n_in, n_out, antialias):
    scale = _F(n_in) / _F(n_out)
    if antialias and scale >= _F(1):
        support, inv = scale, _F(1) / scale
    else:
        support, inv = _F(1), _F(1)
    K = 2 * int(np.ceil(support)) + 1
    center = scale * (np.arange(n_out, dtype=np.float32) + _F(0.5))
    lo = np.maximum(0, ((center - support) + _F(0.5)).astype(np.int32)).astype(np.int32)
    hi = np.minimum(n_in, ((center + support) + _F(0.5)).astype(np.int32)).astype(np.int32)
    count = (hi - lo).astype(np.int32)
    assert count.min() >= 1 and count.max() <= K
    k = np.arange(K, dtype=np.int32)[None, :]
    j = (lo[:, None] + k).astype(np.float32)
    raw = np.maximum(_F(0), _F(1) - np.abs(((j - center[:, None]) + _F(0.5)) * inv)).astype(np.float32)
    raw[k >= count[:, None]] = 0
    tot = np.zeros(n_out, dtype=np.float32)
    for c in range(K):                             # ascending j; the zeros behind `count` add nothing
        tot = tot + raw[:, c]
    weight = (raw / tot[:, None]).astype(np.float32)
    for a in (lo, count, weight):
        a.setflags(write=False)
    return lo, count, weight


def resize_taps(n_in, n_out, antialias):
    """(lo int32 [n_out], count int32 [n_out], weight float32 [n_out, K]) -- module docstring.  The arrays are shared: read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError("resize_taps: sizes are at least 1")
    return _taps(n_in, n_out, bool(antialias))


def _pass(v, taps):
    """The last axis of v (float32 [..., n_in]) through the taps -> float32 [..., n_out]."""
    lo, count, weight = taps
    n_in = v.shape[-1]
    acc = np.zeros(v.shape[:-1] + (len(lo),), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(weight.shape[1]):
            live = k < count
            if not live.any():
                break
            t = v[..., np.minimum(lo + k, n_in - 1)] * weight[:, k]          # the product, rounded
            acc = np.where(live, acc + t, acc)                               # then the sum
    return acc


def resize_with_pad_plan(src_hw, out_hw, side="top_left"):
    """(ox, oy, rw, rh): where the H x W source goes in the out_h x out_w output with its aspect ratio kept.  ratio = max(W / out_w, H / out_h),
    rw = int(W / ratio), rh = int(H / ratio) in Python floats; the padding lies on the left and on top (ox = out_w - rw, oy = out_h - rh), as
    in the VLA policies' resize_with_pad, or, side "center", half of it (rounded down) does."""
    if side not in ("top_left", "center"):
        raise ValueError(f"side {side!r}: 'top_left' or 'center'")
    H, W = int(src_hw[0]), int(src_hw[1])
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if min(H, W, oh, ow) < 1:
        raise ValueError("resize_with_pad_plan: sizes are at least 1")
    ratio = max(W / ow, H / oh)
    rw, rh = max(1, min(ow, int(W / ratio))), max(1, min(oh, int(H / ratio)))
    px, py = ow - rw, oh - rh
    return (px, py, rw, rh) if side == "top_left" else (px // 2, py // 2, rw, rh)


def _three(x, what, default):
    a = np.full(3, default, dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32).reshape(-1)
    if a.shape != (3,):
        raise ValueError(f"image resize: {what} is three values")
    return a


def check_resize(src_shape, src_box, dst, src_index, out_hw, fmt=0, antialias=1, fill=None, mean=None, std=None):
    """The conditions avsim_image_resize puts on its arguments; src_shape = (n, H, W).  Raises ValueError."""
    n, H, W = (int(v) for v in src_shape)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if fmt not in (0, 1):
        raise ValueError("image resize: a format is 0 (u8 HWC) or 1 (float32 CHW)")
    if not (1 <= oh <= 65535 and 1 <= ow <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("image resize: a size outside 1..65535")
    if antialias not in (0, 1):
        raise ValueError("image resize: antialias is 0 or 1")
    if not np.isfinite(_three(fill, "fill", 0)).all():
        raise ValueError("image resize: a fill that is not finite")
    if (mean is None) != (std is None):
        raise ValueError("image resize: mean and std come together")
    if std is not None:
        s = _three(std, "std", 1)
        _three(mean, "mean", 0)
        if not np.isfinite(s).all() or (s == 0).any():
            raise ValueError("image resize: a std that is 0 or not finite")
    b = np.asarray(src_box, dtype=np.int64).reshape(-1, 5)
    d = np.asarray(dst, dtype=np.int64).reshape(-1, 4)
    if n < 1 or len(b) < 1:
        raise ValueError("image resize: no images")
    if len(b) != len(d) or (src_index is not None and len(src_index) != len(b)):
        raise ValueError("image resize: one source box, one dst rectangle and one source index per output")
    for i, ((x0, y0, w, h, flip), (ox, oy, rw, rh)) in enumerate(zip(b, d)):
        s = i if src_index is None else int(src_index[i])
        if not 0 <= s < n:
            raise ValueError(f"image resize: output {i}: source image out of range")
        if w < 1 or h < 1 or rw < 1 or rh < 1:
            raise ValueError(f"image resize: output {i}: an empty source box or dst rectangle")
        if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError(f"image resize: output {i}: the source box does not lie inside the image")
        if ox < 0 or oy < 0 or ox + rw > ow or oy + rh > oh:
            raise ValueError(f"image resize: output {i}: the dst rectangle does not lie inside the output")
        if w > MAX_RATIO * rw or h > MAX_RATIO * rh:
            raise ValueError(f"image resize: output {i}: a ratio above {MAX_RATIO}")
        if flip not in (0, 1):
            raise ValueError(f"image resize: output {i}: flip is 0 or 1")


def resize_reference(img, fmt, src_box, dst, out_hw, antialias=1, fill=None, mean=None, std=None, src_index=None):
    """float32 [nout, 3, out_h, out_w] (module docstring)."""
    a = np.asarray(img)
    if fmt == 0 and a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3:
        n, H, W = a.shape[:3]
    elif fmt == 1 and a.dtype == np.float32 and a.ndim == 4 and a.shape[1] == 3:
        n, H, W = a.shape[0], a.shape[2], a.shape[3]
    else:
        raise ValueError("image resize: images are uint8 [n, H, W, 3] (fmt 0) or float32 [n, 3, H, W] (fmt 1)")
    b = np.asarray(src_box, dtype=np.int64).reshape(-1, 5)
    d = np.asarray(dst, dtype=np.int64).reshape(-1, 4)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    check_resize((n, H, W), b, d, src_index, (oh, ow), fmt, antialias, fill, mean, std)
    fill = _three(fill, "fill", 0)
    table = np.arange(256, dtype=np.float32) / _F(255)
    out = np.empty((len(b), 3, oh, ow), dtype=np.float32)
    out[:] = fill[None, :, None, None]
    for i, ((x0, y0, w, h, flip), (ox, oy, rw, rh)) in enumerate(zip(b, d)):
        s = i if src_index is None else int(src_index[i])
        if fmt == 0:
            reg = table[a[s, y0:y0 + h, x0:x0 + w]].transpose(2, 0, 1)                  # [3, h, w]
        else:
            reg = a[s, :, y0:y0 + h, x0:x0 + w]
        t = _pass(reg, resize_taps(w, rw, antialias))                                   # [3, h, rw]
        r = _pass(t.transpose(0, 2, 1), resize_taps(h, rh, antialias)).transpose(0, 2, 1)      # [3, rh, rw]
        out[i, :, oy:oy + rh, ox:ox + rw] = r[:, :, ::-1] if flip else r
    if mean is not None:
        m, sd = _three(mean, "mean", 0), _three(std, "std", 1)
        with np.errstate(invalid="ignore", over="ignore"):
            out = ((out - m[None, :, None, None]) / sd[None, :, None, None]).astype(np.float32)
    return out


def mean_std(mean, std):
    """float32 [2, 3] for the C call, or None."""
    if (mean is None) != (std is None):
        raise ValueError("image resize: mean and std come together")
    if mean is None:
        return None
    return np.ascontiguousarray(np.stack([_three(mean, "mean", 0), _three(std, "std", 1)]), dtype=np.float32)


def boxes(crop_box, crop_hw, out_hw, mode="stretch", side="top_left"):
    """(src_box int32 [n, 5], dst int32 [n, 4]) of crop boxes (x0, y0, flip) of size crop_hw resized into out_hw: "stretch" fills the output,
    "pad" keeps the aspect ratio (resize_with_pad_plan)."""
    if mode not in ("stretch", "pad"):
        raise ValueError(f"resize_mode {mode!r}: 'stretch' or 'pad'")
    cb = np.asarray(crop_box, dtype=np.int32).reshape(-1, 3)
    h, w = int(crop_hw[0]), int(crop_hw[1])
    sb = np.empty((len(cb), 5), dtype=np.int32)
    sb[:, 0], sb[:, 1], sb[:, 2], sb[:, 3], sb[:, 4] = cb[:, 0], cb[:, 1], w, h, cb[:, 2]
    rect = (0, 0, int(out_hw[1]), int(out_hw[0])) if mode == "stretch" else resize_with_pad_plan((h, w), out_hw, side)
    return sb, np.tile(np.array([rect], dtype=np.int32), (len(cb), 1))
