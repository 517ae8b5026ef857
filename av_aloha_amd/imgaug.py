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
op that was not chosen is its identity (1, 1, 1, 0, 1) and its bit is clear.

The geometric op (avsim_image_augment; torchvision's RandomAffine, fill 0) is bit 5, AFFINE = 32.  It runs after the five colour
ops, on the WHOLE source image, before the box is cut and before the normalisation (so fill pixels are normalised too).  An output has a
float32 inverse matrix M[6] and the call one interp (0 nearest, 1 bilinear).  For the pixel (x, y) of the H x W image, every operation
float32 and rounded on its own:
  xf = (float32(x) + 0.5) - float32(W) / 2,    yf = (float32(y) + 0.5) - float32(H) / 2
  sx = (((M0 * xf) + (M1 * yf)) + M2) + (float32(W) / 2 - 0.5),    sy = (((M3 * xf) + (M4 * yf)) + M5) + (float32(H) / 2 - 0.5)
  nearest    the tap (rint(sx), rint(sy)), half to even
  bilinear   x0 = floor(sx), wx = sx - x0, y0 = floor(sy), wy = sy - y0; the taps t00 = (x0, y0), t01 = (x0 + 1, y0), t10 = (x0, y0 + 1),
             t11 = (x0 + 1, y0 + 1); top = t00 * (1 - wx) + t01 * wx, bot = t10 * (1 - wx) + t11 * wx, v = top * (1 - wy) + bot * wy
  a tap (xi, yi) is inside iff 0 <= xi <= W - 1 and 0 <= yi <= H - 1, tested on the FLOAT values before any conversion to an integer;
  a tap that is not inside is 0.0 in all channels (torchvision's fill=0, grid_sample(padding_mode="zeros", align_corners=False)).
affine_matrix is torchvision's _get_inverse_affine_matrix with the centre at the origin, in float64, rounded to float32 at the end.

The plan with the geometric op (augment_plan_affine): the same stream as augment_plan.  With an "affine" entry of weight > 0 the choice is
rng.choice(6, ...) over the six ops, and after the chosen colour ops' uniforms a chosen affine draws, in this order: the angle
uniform(degrees); with a translate: tx = rint(uniform(-tr_x W, tr_x W)), then ty = rint(uniform(-tr_y H, tr_y H)); with a scale range:
uniform(scale); with a shear range: uniform(shear[0:2]) for x, then, with four values, uniform(shear[2:4]) for y.  Without the entry, or
with weight 0, the draws are augment_plan's."""
import math

import numpy as np

OPS = ("brightness", "contrast", "saturation", "hue", "sharpness")
BRIGHTNESS, CONTRAST, SATURATION, HUE, SHARPNESS = 1, 2, 4, 8, 16
AFFINE = 32
IDENTITY = np.array([1, 1, 1, 0, 1], dtype=np.float32)
IDENTITY_MATRIX = np.array([1, 0, 0, 0, 1, 0], dtype=np.float32)
IDENTITY_DRAWN = np.array([0, 0, 0, 1, 0, 0], dtype=np.float64)      # angle, tx, ty, scale, shear_x, shear_y
MATRIX_LIMIT = float(1 << 20)                                        # the largest magnitude of a matrix entry avsim_image_augment takes
INTERPOLATIONS = ("nearest", "bilinear")
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
    """DEFAULT_CFG with the fields of `cfg` (a dict, True or None) laid over it; ValueError for what avsim_image_jitter would refuse.  An
    "affine" entry (_affine_cfg) is kept, checked and completed; without one the result has no such key."""
    out = {k: (dict(v) if isinstance(v, dict) else v) for k, v in DEFAULT_CFG.items()}
    if isinstance(cfg, dict):
        for k, v in cfg.items():
            if k == "affine":
                out[k] = _affine_cfg(v)
                continue
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


def _affine_cfg(v):
    """The "affine" entry of a config with its defaults (LeRobot's: degrees (-5, 5), translate (0.05, 0.05), no scale, no shear, nearest)
    laid under it: weight, degrees (lo, hi), translate (tr_x, tr_y) or None, scale (lo, hi) or None, shear () or (x lo, x hi) or
    (x lo, x hi, y lo, y hi), interpolation "nearest" / "bilinear"."""
    if not isinstance(v, dict):
        raise ValueError("augment: affine: a dict")
    if set(v) - {"weight", "degrees", "translate", "scale", "shear", "interpolation"}:
        raise ValueError("augment: affine: the fields are 'weight', 'degrees', 'translate', 'scale', 'shear' and 'interpolation'")
    a = {"weight": 1.0, "degrees": (-5.0, 5.0), "translate": (0.05, 0.05), "scale": None, "shear": None, "interpolation": "nearest"}
    a.update(v)
    w = float(a["weight"])
    if not (np.isfinite(w) and w >= 0):
        raise ValueError(f"augment: affine: weight {w}")
    d = a["degrees"]
    d = (-float(d), float(d)) if np.isscalar(d) else tuple(float(x) for x in d)
    if not (len(d) == 2 and -360.0 <= d[0] <= d[1] <= 360.0):
        raise ValueError(f"augment: affine: degrees {d}")
    t = a["translate"]
    if t is not None:
        t = tuple(float(x) for x in t)
        if not (len(t) == 2 and all(0.0 <= x <= 1.0 for x in t)):
            raise ValueError(f"augment: affine: translate {t}: two fractions in [0, 1]")
    sc = a["scale"]
    if sc is not None:
        sc = tuple(float(x) for x in sc)
        if not (len(sc) == 2 and 2.0 ** -8 <= sc[0] <= sc[1] <= 2.0 ** 8):
            raise ValueError(f"augment: affine: scale {sc}: a range inside [2^-8, 2^8]")
    sh = a["shear"]
    if sh is not None:
        sh = (-float(sh), float(sh)) if np.isscalar(sh) else tuple(float(x) for x in sh)
        if not (len(sh) in (2, 4) and all(-80.0 <= x <= 80.0 for x in sh) and sh[0] <= sh[1] and (len(sh) == 2 or sh[2] <= sh[3])):
            raise ValueError(f"augment: affine: shear {sh}: (lo, hi) or (x lo, x hi, y lo, y hi) in degrees within +-80")
    if a["interpolation"] not in INTERPOLATIONS:
        raise ValueError(f"augment: affine: interpolation {a['interpolation']!r}: 'nearest' or 'bilinear'")
    return {"weight": w, "degrees": d, "translate": t, "scale": sc, "shear": sh, "interpolation": a["interpolation"]}


def has_affine(cfg):
    """Whether a make_cfg result chooses the geometric op at all."""
    return cfg is not None and "affine" in cfg and cfg["affine"]["weight"] > 0


def interp_of(cfg):
    """The `interp` of avsim_image_augment for a make_cfg result: 0 nearest, 1 bilinear."""
    return INTERPOLATIONS.index(cfg["affine"]["interpolation"]) if cfg is not None and "affine" in cfg else 0


def augment_plan(n_images, cfg=None, seed=0, epoch=0, batch=0, camera_index=0):
    """(mask int32 [n_images], factor float32 [n_images, 5]) of one camera's images of one batch (module docstring for the draws).  The five
    colour ops only: an "affine" entry of cfg is not looked at (augment_plan_affine is the plan that has it)."""
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


LEROBOT_CFG = dict(DEFAULT_CFG, affine={"weight": 1.0, "degrees": (-5.0, 5.0), "translate": (0.05, 0.05), "interpolation": "nearest"})


def affine_matrix(angle_deg, tx=0.0, ty=0.0, scale=1.0, shear_x_deg=0.0, shear_y_deg=0.0):
    """float32 [6]: affine_matrix64 rounded to float32, what avsim_image_augment takes."""
    return affine_matrix64(angle_deg, tx, ty, scale, shear_x_deg, shear_y_deg).astype(np.float32)


def affine_matrix64(angle_deg, tx=0.0, ty=0.0, scale=1.0, shear_x_deg=0.0, shear_y_deg=0.0):
    """float64 [6]: the inverse matrix (output pixel -> source pixel, both relative to the image centre) of a rotation by angle_deg
    (clockwise on the screen), a scale, shears and then a translation by (tx, ty) pixels: torchvision's _get_inverse_affine_matrix with
    the centre at the origin, in float64, every step written out."""
    rot, sx, sy = math.radians(float(angle_deg)), math.radians(float(shear_x_deg)), math.radians(float(shear_y_deg))
    tx, ty, scale = float(tx), float(ty), float(scale)
    # the forward rotation-shear [[a, b], [c, d]] = R(rot) SHy(sy) SHx(sx), whose determinant is 1
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    # its inverse over the scale, then the inverse of the translation
    m = [d / scale, -b / scale, 0.0, -c / scale, a / scale, 0.0]
    m[2] += m[0] * (-tx) + m[1] * (-ty)
    m[5] += m[3] * (-tx) + m[4] * (-ty)
    return np.array(m, dtype=np.float64)


def _source_coords(H, W, M):
    """(sx, sy) float32 [H, W] of the module docstring."""
    M = np.asarray(M, dtype=np.float32).reshape(6)
    half_w, half_h = np.float32(W) / np.float32(2), np.float32(H) / np.float32(2)
    xf = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) - half_w)[None, :]
    yf = ((np.arange(H, dtype=np.float32) + np.float32(0.5)) - half_h)[:, None]
    sx = (((M[0] * xf) + (M[1] * yf)) + M[2]) + (half_w - np.float32(0.5))
    sy = (((M[3] * xf) + (M[4] * yf)) + M[5]) + (half_h - np.float32(0.5))
    return sx.astype(np.float32), sy.astype(np.float32)


def _tap(x, xi, yi):
    """float32 [H, W, 3]: x at the float tap coordinates (xi, yi), 0.0 where the tap is not inside."""
    H, W = x.shape[:2]
    inside = (xi >= _0) & (xi <= np.float32(W - 1)) & (yi >= _0) & (yi <= np.float32(H - 1))
    ix = np.where(inside, xi, _0).astype(np.int64)
    iy = np.where(inside, yi, _0).astype(np.int64)
    return np.where(inside[..., None], x[iy, ix], _0).astype(np.float32)


def affine_reference(x, M, interp=0):
    """float32 [H, W, 3]: the float image x resampled through the inverse matrix M (module docstring)."""
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[:2]
    if interp not in (0, 1):
        raise ValueError("image augment: interp is 0 (nearest) or 1 (bilinear)")
    with np.errstate(over="ignore", invalid="ignore"):
        sx, sy = _source_coords(H, W, M)
        if interp == 0:
            return _tap(x, np.rint(sx), np.rint(sy))
        x0, y0 = np.floor(sx), np.floor(sy)
        wx, wy = (sx - x0)[..., None], (sy - y0)[..., None]
        x1, y1 = x0 + _1, y0 + _1
        top = _tap(x, x0, y0) * (_1 - wx) + _tap(x, x1, y0) * wx
        bot = _tap(x, x0, y1) * (_1 - wx) + _tap(x, x1, y1) * wx
        return (top * (_1 - wy) + bot * wy).astype(np.float32)


def check_jitter_affine(src_shape, params, matrix, interp, out_hw, mean=None, std=None, src_index=None):
    """The conditions avsim_image_augment puts on its arguments (include/avsim.h); raises ValueError.  check_jitter's, with masks 0..63,
    interp 0 / 1 and, for an output whose bit 5 is set, six finite matrix entries of magnitude at most 2^20 (the entries of an output
    without the bit are not read; matrix may be None when no output has it)."""
    bm, fac = split_params(params)
    if interp not in (0, 1):
        raise ValueError("image augment: interp is 0 (nearest) or 1 (bilinear)")
    mask = bm[:, 3].astype(np.int64)
    for i, m in enumerate(mask.tolist()):
        if not 0 <= m <= 63:
            raise ValueError(f"image augment: output {i}: mask outside 0..63")
    colour = bm.copy()
    colour[:, 3] &= 31
    check_jitter(src_shape, (colour, fac), out_hw, mean, std, src_index)
    if (mask & AFFINE).any():
        if matrix is None:
            raise ValueError("image augment: an output has bit 5 and there are no matrices")
        mat = np.asarray(matrix, dtype=np.float32).reshape(len(bm), 6)
        for i in np.nonzero(mask & AFFINE)[0].tolist():
            if not (np.isfinite(mat[i]).all() and (np.abs(mat[i]) <= np.float32(MATRIX_LIMIT)).all()):
                raise ValueError(f"image augment: output {i}: a matrix entry that is not finite or beyond 2^20 in magnitude")


def jitter_affine_reference(img_u8, params, matrix, interp, out_hw, mean=None, std=None, src_index=None):
    """float32 [nout, 3, oh, ow]: jitter_reference with the geometric op (module docstring): the colour ops of mask & 31 on the whole image,
    affine_reference where bit 5 is set, the box, the normalisation.  matrix: float32 [nout, 6], or None when no mask has bit 5."""
    u = np.asarray(img_u8)
    if not (u.dtype == np.uint8 and u.ndim == 4 and u.shape[3] == 3):
        raise ValueError("image augment: images are uint8 [n, H, W, 3]")
    bm, fac = split_params(params)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    check_jitter_affine(u.shape[:3], (bm, fac), matrix, interp, (oh, ow), mean, std, src_index)
    mat = None if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(len(bm), 6)
    out = np.empty((len(bm), 3, oh, ow), dtype=np.float32)
    if std is not None:
        m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
        s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    done = {}
    for i, ((x0, y0, flip, mask), f) in enumerate(zip(bm.tolist(), fac)):
        src = i if src_index is None else int(src_index[i])
        key = (src, mask & 31, tuple(f[k].tobytes() for k in range(5) if mask >> k & 1))
        if key not in done:
            done[key] = apply_ops(u[src], mask & 31, f)
        x = done[key]
        if mask & AFFINE:
            x = affine_reference(x, mat[i], interp)
        crop = x[y0:y0 + oh, x0:x0 + ow]
        if flip:
            crop = crop[:, ::-1]
        v = np.transpose(crop, (2, 0, 1))
        out[i] = (v - m) / s if std is not None else v
    return out


def augment_plan_affine(n_images, cfg=None, seed=0, epoch=0, batch=0, camera_index=0, size=None):
    """(mask int32 [n], factor float32 [n, 5], matrix float32 [n, 6], drawn float64 [n, 6] = (angle, tx, ty, scale, shear_x, shear_y)) of
    one camera's images of one batch (module docstring for the draws); size = (H, W) of the camera's images.  An image whose bit 5 is clear
    has the identity matrix and the identity draw (0, 0, 0, 1, 0, 0).  Without an "affine" entry of weight > 0 the first two results are
    augment_plan's, bit for bit and draw for draw."""
    cfg = make_cfg(cfg)
    n = int(n_images)
    matrix, drawn = np.tile(IDENTITY_MATRIX, (n, 1)), np.tile(IDENTITY_DRAWN, (n, 1))
    if not has_affine(cfg):
        return augment_plan(n, cfg, seed, epoch, batch, camera_index) + (matrix, drawn)
    if size is None:
        raise ValueError("augment_plan_affine: size=(H, W) of the images")
    H, W = int(size[0]), int(size[1])
    aff = cfg["affine"]
    rng = np.random.default_rng([int(seed), int(epoch), 1, int(batch), int(camera_index)])
    w = np.array([float(cfg[name]["weight"]) for name in OPS] + [aff["weight"]], dtype=np.float64)
    k = min(int(cfg["max_num_transforms"]), int((w > 0).sum()))
    mask = np.zeros(n, dtype=np.int32)
    factor = np.tile(IDENTITY, (n, 1))
    if k == 0:
        return mask, factor, matrix, drawn
    p = w / w.sum()
    for i in range(n):
        chosen = sorted(int(c) for c in rng.choice(6, size=k, replace=False, p=p))
        for op in chosen:
            mask[i] |= 1 << op
            if op < 5:
                lo, hi = cfg[OPS[op]]["min_max"]
                factor[i, op] = np.float32(rng.uniform(float(lo), float(hi)))
                continue
            d = drawn[i]
            d[0] = rng.uniform(*aff["degrees"])
            if aff["translate"] is not None:
                mx, my = aff["translate"][0] * W, aff["translate"][1] * H
                d[1] = np.rint(rng.uniform(-mx, mx))
                d[2] = np.rint(rng.uniform(-my, my))
            if aff["scale"] is not None:
                d[3] = rng.uniform(*aff["scale"])
            if aff["shear"] is not None:
                d[4] = rng.uniform(aff["shear"][0], aff["shear"][1])
                if len(aff["shear"]) == 4:
                    d[5] = rng.uniform(aff["shear"][2], aff["shear"][3])
            matrix[i] = affine_matrix(*d)
    return mask, factor, matrix, drawn
