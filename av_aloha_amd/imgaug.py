"""Colour and sharpness augmentation of training images: the specification of avsim_image_jitter (csrc/avsim_imgaug.hip) in numpy, bit for
bit, and the random plan that chooses the operations.  The arithmetic is torchvision's documented adjust_brightness /
adjust_contrast / adjust_saturation / adjust_hue / adjust_sharpness for float images, the subset, order and ranges are LeRobot's
image_transforms.

Every operation below is one float32 operation rounded on its own: no fused multiply-add, no float64 (but for the contrast mean, stated
there).  Selections are np.where, never a multiplication by a mask.  clamp(x) = where(x < 0, 0, where(x > 1, 1, x)).

An image is u8 [H, W, 3]; its float value is p = float32(u) / float32(255).  An output has an op mask (bit 0 brightness, 1 contrast,
2 saturation, 3 hue, 4 sharpness) and five factors (fb, fc, fs, fh, fsh).  The ops whose bits are set are applied in that order to the WHOLE
source image, floats carried from op to op and never requantised; then the box (x0, y0, flip) is cut (as imgprep.prep_reference cuts it);
then every channel is normalised as (v - mean[c]) / std[c], or left in [0, 1] without mean / std.

  blend(a, b, f) = clamp(a * f + b * (float32(1) - f))        two products, then one sum
  gray(x)        = (0.2989 * r + 0.587 * g) + 0.114 * b
  brightness     blend(p, 0, fb)
  contrast       blend(x, m, fc), m the mean of gray(x) over the H * W pixels of the source image (x: after brightness if its bit is set).
                 So that the mean has no summation order: q = uint32(gray * float32(1048576) + float32(0.5)) per pixel, S = the integer sum of
                 q, m = float32(float64(S) / float64(H * W * 1048576)).  m is within 2^-21 of the float64 mean of gray (torchvision's own
                 float32 mean is no closer to it)
  saturation     blend(x, gray(x), fs) per pixel
  hue            torchvision's _rgb_to_hsv, h = h + fh, h = h - floor(h), _hsv_to_rgb, every step written out in _hue below
  sharpness      for a pixel that is not on the source image's first or last row or column: t = the sum of its eight neighbours of x, added in
                 the order row above left to right, left, right, row below left to right, every addition rounded;
                 blur = (t + float32(5) * c) / float32(13); the result is blend(x, blur, fsh).  A border pixel keeps x (so an image with H < 3
                 or W < 3 is unchanged); the border is the source image's, not the crop's.  torchvision's convolution sums the same nine
                 products (kernel 1/13, centre 5/13) in another, unspecified order: it differs from this by rounding only.

The plan (augment_plan): rng = np.random.default_rng([seed, epoch, 1, batch, camera_index]) -- a stream of its own, dataset.epoch_plan's
([seed, epoch]) is untouched.  cfg holds, per op, "weight" and "min_max", and "max_num_transforms"; the defaults are LeRobot's.  With
ops = those of weight > 0 and k = min(max_num_transforms, len(ops)), the draws are, image after image: first
rng.choice(5, size=k, replace=False, p=weight / weight.sum()) (nothing drawn when k = 0), then one rng.uniform(min, max) for every chosen op
in the canonical order brightness, contrast, saturation, hue, sharpness (LeRobot's random_order=False), stored as float32.  The factor of an
op that was not chosen is its identity (1, 1, 1, 0, 1) and its bit is clear."""
import numpy as np

OPS = ("brightness", "contrast", "saturation", "hue", "sharpness")
BRIGHTNESS, CONTRAST, SATURATION, HUE, SHARPNESS = 1, 2, 4, 8, 16
IDENTITY = np.array([1, 1, 1, 0, 1], dtype=np.float32)
GRAY_SCALE = 1048576            # 2^20: the fixed point of the contrast mean

PARAMS_DTYPE = np.dtype([("x0", np.int32), ("y0", np.int32), ("flip", np.int32), ("mask", np.int32), ("factor", np.float32, (5,))])

DEFAULT_CFG = {
    "max_num_transforms": 3,
    "brightness": {"weight": 1.0, "min_max": (0.8, 1.2)},
    "contrast": {"weight": 1.0, "min_max": (0.8, 1.2)},
    "saturation": {"weight": 1.0, "min_max": (0.5, 1.5)},
    "hue": {"weight": 1.0, "min_max": (-0.05, 0.05)},
    "sharpness": {"weight": 1.0, "min_max": (0.8, 1.2)},
}

_0, _1 = np.float32(0), np.float32(1)


def split_params(params):
    """(box_mask int32 [nout, 4] = (x0, y0, flip, mask), factor float32 [nout, 5]) of a PARAMS_DTYPE array or of such a pair."""
    if isinstance(params, np.ndarray) and params.dtype.names:
        p = params.reshape(-1)
        bm = np.stack([p["x0"], p["y0"], p["flip"], p["mask"]], axis=1).astype(np.int32)
        return np.ascontiguousarray(bm), np.ascontiguousarray(p["factor"], dtype=np.float32).reshape(-1, 5)
    bm, f = params
    bm = np.ascontiguousarray(bm, dtype=np.int32).reshape(-1, 4)
    return bm, np.ascontiguousarray(f, dtype=np.float32).reshape(len(bm), 5)


def pack_params(box, mask, factor):
    """The pair split_params returns, from boxes int [nout, 3] = (x0, y0, flip) and augment_plan's (mask, factor)."""
    box = np.asarray(box, dtype=np.int32).reshape(-1, 3)
    bm = np.concatenate([box, np.asarray(mask, dtype=np.int32).reshape(-1, 1)], axis=1)
    return np.ascontiguousarray(bm), np.ascontiguousarray(factor, dtype=np.float32).reshape(len(bm), 5)


def mean_std(mean, std):
    """float32 [2, 3] = (mean, std) as avsim_image_jitter takes them, or None when both are None."""
    if mean is None and std is None:
        return None
    if mean is None or std is None:
        raise ValueError("image jitter: mean and std come together")
    return np.ascontiguousarray(np.stack([np.asarray(mean, dtype=np.float32).reshape(3), np.asarray(std, dtype=np.float32).reshape(3)]))


def clamp(x):
    return np.where(x < _0, _0, np.where(x > _1, _1, x)).astype(np.float32)


def blend(a, b, f):
    f = np.float32(f)
    return clamp(a * f + b * (_1 - f))


def gray(x):
    """float32 [..., 3] -> [...]."""
    return (np.float32(0.2989) * x[..., 0] + np.float32(0.587) * x[..., 1]) + np.float32(0.114) * x[..., 2]


def to_float(img_u8):
    return img_u8.astype(np.float32) / np.float32(255)


def _gray_sum(x):
    q = (gray(x) * np.float32(GRAY_SCALE) + np.float32(0.5)).astype(np.uint32)
    return int(q.sum(dtype=np.uint64))


def gray_mean(x):
    """The contrast mean m of a float image [H, W, 3] (module docstring)."""
    n = x.shape[0] * x.shape[1]
    return np.float32(np.float64(_gray_sum(x)) / np.float64(n * GRAY_SCALE))


def _hue(x, fh):
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    # _rgb_to_hsv
    maxc = np.maximum(np.maximum(r, g), b)
    minc = np.minimum(np.minimum(r, g), b)
    eqc = maxc == minc
    cr = maxc - minc
    s = cr / np.where(eqc, _1, maxc)
    crd = np.where(cr == _0, _1, cr)
    rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
    h = np.where(maxc == r, bc - gc, np.where(maxc == g, np.float32(2) + rc - bc, np.float32(4) + gc - rc))
    h = h / np.float32(6) + _1
    h = h - np.floor(h)
    # the shift
    h = h + np.float32(fh)
    h = h - np.floor(h)
    # _hsv_to_rgb
    v = maxc
    h6 = h * np.float32(6)
    fl = np.floor(h6)
    f = h6 - fl
    i = fl.astype(np.int32) % 6
    p = clamp(v * (_1 - s))
    q = clamp(v * (_1 - s * f))
    t = clamp(v * (_1 - s * (_1 - f)))

    def six(a0, a1, a2, a3, a4, a5):
        return np.where(i == 0, a0, np.where(i == 1, a1, np.where(i == 2, a2, np.where(i == 3, a3, np.where(i == 4, a4, a5)))))

    return np.stack([six(v, q, p, p, t, v), six(t, v, v, q, p, p), six(p, p, t, v, v, q)], axis=-1).astype(np.float32)


def _sharpness(x, fsh):
    H, W = x.shape[:2]
    if H < 3 or W < 3:
        return x
    c = x[1:-1, 1:-1]
    t = x[:-2, :-2] + x[:-2, 1:-1]
    for nb in (x[:-2, 2:], x[1:-1, :-2], x[1:-1, 2:], x[2:, :-2], x[2:, 1:-1], x[2:, 2:]):
        t = t + nb
    blur = (t + np.float32(5) * c) / np.float32(13)
    out = x.copy()
    out[1:-1, 1:-1] = blend(c, blur, fsh)
    return out


def apply_ops(img_u8, mask, factor):
    """float32 [H, W, 3]: the ops of `mask` applied to the whole image u8 [H, W, 3]."""
    x = to_float(np.asarray(img_u8))
    fb, fc, fs, fh, fsh = (np.float32(v) for v in factor)
    if mask & BRIGHTNESS:
        x = blend(x, _0, fb)
    if mask & CONTRAST:
        x = blend(x, gray_mean(x), fc)
    if mask & SATURATION:
        x = blend(x, gray(x)[..., None], fs)
    if mask & HUE:
        x = _hue(x, fh)
    if mask & SHARPNESS:
        x = _sharpness(x, fsh)
    return x


def check_jitter(src_shape, params, out_hw, mean=None, std=None, src_index=None):
    """The conditions avsim_image_jitter puts on its arguments (include/avsim.h); raises ValueError.  src_shape: (nsrc, H, W)."""
    n, H, W = (int(v) for v in src_shape)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    bm, fac = split_params(params)
    if n < 1 or len(bm) < 1:
        raise ValueError("image jitter: nsrc and nout are at least 1")
    if not (1 <= oh <= 65535 and 1 <= ow <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("image jitter: a size outside 1..65535")
    if (mean is None) != (std is None):
        raise ValueError("image jitter: mean and std come together")
    if std is not None:
        s = np.asarray(std, dtype=np.float32).reshape(-1)
        m = np.asarray(mean, dtype=np.float32).reshape(-1)
        if s.shape != (3,) or m.shape != (3,):
            raise ValueError("image jitter: mean and std hold three values")
        if not np.isfinite(s).all() or (s == 0).any():
            raise ValueError("image jitter: a std that is 0 or not finite")
    for i, ((x0, y0, flip, mask), f) in enumerate(zip(bm.astype(np.int64), fac)):
        s = i if src_index is None else int(src_index[i])
        if not 0 <= s < n:
            raise ValueError(f"image jitter: output {i}: source image out of range")
        if flip not in (0, 1):
            raise ValueError(f"image jitter: output {i}: flip is 0 or 1")
        if not 0 <= mask <= 31:
            raise ValueError(f"image jitter: output {i}: mask outside 0..31")
        if x0 < 0 or y0 < 0 or x0 + ow > W or y0 + oh > H:
            raise ValueError(f"image jitter: output {i}: the crop does not lie inside the source")
        for k, name in enumerate(OPS):
            if not mask >> k & 1:
                continue                                # factors of unset bits are not looked at
            if not np.isfinite(f[k]):
                raise ValueError(f"image jitter: output {i}: the {name} factor is not finite")
            lo, hi = (-0.5, 0.5) if k == 3 else (0.0, 16.0)
            if not lo <= f[k] <= hi:
                raise ValueError(f"image jitter: output {i}: the {name} factor {f[k]} outside [{lo}, {hi}]")


def jitter_reference(img_u8, params, out_hw, mean=None, std=None, src_index=None):
    """float32 [nout, 3, oh, ow] (module docstring).  img_u8: u8 [nsrc, H, W, 3]; params: split_params'; mean / std: three values each, or
    None: the output stays in [0, 1]; src_index: int [nout] or None (output i reads image i)."""
    u = np.asarray(img_u8)
    if not (u.dtype == np.uint8 and u.ndim == 4 and u.shape[3] == 3):
        raise ValueError("image jitter: images are uint8 [n, H, W, 3]")
    bm, fac = split_params(params)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    check_jitter(u.shape[:3], (bm, fac), (oh, ow), mean, std, src_index)
    out = np.empty((len(bm), 3, oh, ow), dtype=np.float32)
    if std is not None:
        m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
        s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    done = {}                                           # (source, mask, the factors looked at) -> the whole image: batches repeat them
    for i, ((x0, y0, flip, mask), f) in enumerate(zip(bm.tolist(), fac)):
        src = i if src_index is None else int(src_index[i])
        key = (src, mask, tuple(f[k].tobytes() for k in range(5) if mask >> k & 1))
        if key not in done:
            done[key] = apply_ops(u[src], mask, f)
        crop = done[key][y0:y0 + oh, x0:x0 + ow]
        if flip:
            crop = crop[:, ::-1]
        v = np.transpose(crop, (2, 0, 1))
        out[i] = (v - m) / s if std is not None else v
    return out


def gray_sum_reference(img_u8, params, src_index=None):
    """uint64 [nout]: the S behind every output's contrast mean -- of the image after brightness where that bit is set (whether or not the
    contrast bit is: the device computes it for the outputs that have it)."""
    u = np.asarray(img_u8)
    bm, fac = split_params(params)
    out = np.empty(len(bm), dtype=np.uint64)
    for i, (mask, f) in enumerate(zip(bm[:, 3].tolist(), fac)):
        x = to_float(u[i if src_index is None else int(src_index[i])])
        if mask & BRIGHTNESS:
            x = blend(x, _0, f[0])
        out[i] = _gray_sum(x)
    return out


def make_cfg(cfg=None):
    """DEFAULT_CFG with the fields of `cfg` (a dict, True or None) laid over it; ValueError for what avsim_image_jitter would refuse."""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULT_CFG.items()}
    if isinstance(cfg, dict):
        for k, v in cfg.items():
            if k not in out:
                raise ValueError(f"augment: unknown field {k!r}")
            if isinstance(v, dict):
                if set(v) - {"weight", "min_max"}:
                    raise ValueError(f"augment: {k}: the fields are 'weight' and 'min_max'")
                out[k].update(v)
            else:
                out[k] = v
    elif cfg not in (None, True):
        raise ValueError("augment: None, True or a dict")
    if int(out["max_num_transforms"]) < 0:
        raise ValueError("augment: max_num_transforms is not negative")
    for k, name in enumerate(OPS):
        w, (lo, hi) = float(out[name]["weight"]), (float(v) for v in out[name]["min_max"])
        band = (-0.5, 0.5) if k == 3 else (0.0, 16.0)
        if not (np.isfinite(w) and w >= 0):
            raise ValueError(f"augment: {name}: weight {w}")
        if not band[0] <= lo <= hi <= band[1]:
            raise ValueError(f"augment: {name}: range ({lo}, {hi}) outside [{band[0]}, {band[1]}]")
    return out


def augment_plan(n_images, cfg=None, seed=0, epoch=0, batch=0, camera_index=0):
    """(mask int32 [n_images], factor float32 [n_images, 5]) of one camera's images of one batch (module docstring for the draws)."""
    cfg = make_cfg(cfg)
    rng = np.random.default_rng([int(seed), int(epoch), 1, int(batch), int(camera_index)])
    w = np.array([float(cfg[name]["weight"]) for name in OPS], dtype=np.float64)
    k = min(int(cfg["max_num_transforms"]), int((w > 0).sum()))
    mask = np.zeros(int(n_images), dtype=np.int32)
    factor = np.tile(IDENTITY, (int(n_images), 1))
    if k == 0:
        return mask, factor
    p = w / w.sum()
    for i in range(int(n_images)):
        chosen = rng.choice(5, size=k, replace=False, p=p)
        for op in sorted(int(c) for c in chosen):
            lo, hi = cfg[OPS[op]]["min_max"]
            factor[i, op] = np.float32(rng.uniform(float(lo), float(hi)))
            mask[i] |= 1 << op
    return mask, factor
