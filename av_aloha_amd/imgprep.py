"""Training batches: the specification of the device's image statistics and image preparation (avsim_image_stats / avsim_image_prep,
csrc/avsim_imgprep.hip.h) in numpy, bit for bit, and the index arithmetic of action chunks.

* `to_u8`: the u8 view of the library's two image formats -- u8 [n, H, W, 3] as it is, float32 [n, 3, H, W] through the encoder's rule
  (int)(v * 255 + 0.5f) in float32 (which gives u back for v = float32(u) / float32(255): the decoder's float output round-trips).
* `stats_reference`: per image and channel (sum, sum of squares, min, max) of the u8 values, as integers; `combine_stats` turns them into a
  data set's mean / std / min / max in [0, 1] by exact rational arithmetic, each value rounded once to float64 and then to float32.  No
  float is accumulated anywhere, so there is no tolerance to state.  std is the population std, as LeRobot's compute_stats uses.
* `normalise_lut`, `identity_lut`: the tables; `prep_reference`: crop + optional mirror + look-up,
  out[i, c, y, x] = lut[lut_index[i], c, u8(img[i])[y0 + y, x0 + (flip ? ow - 1 - x : x), c]].
* `chunk_index`: LeRobot's delta_timestamps clamping -- the frames of an action chunk and which of them are padding; `history_index`:
  the same for the frames in front of one (n_obs_steps > 1)."""
from fractions import Fraction

import numpy as np


def to_u8(img):
    """u8 [n, H, W, 3] of an image batch in either format."""
    a = np.asarray(img)
    if a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3:
        return a
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[1] == 3:
        y = a * np.float32(255) + np.float32(0.5)              # each operation rounded to float32 on its own
        with np.errstate(invalid="ignore"):
            y = np.minimum(np.maximum(y, np.float32(0)), np.float32(255))
        return np.ascontiguousarray(np.nan_to_num(y, nan=0.0).astype(np.int32).astype(np.uint8).transpose(0, 2, 3, 1))
    raise ValueError("images are uint8 [n, H, W, 3] or float32 [n, 3, H, W]")


def stats_reference(img, index=None):
    """uint64 [n, 3, 4]: (sum, sum of squares, min, max) of the u8 values per image (index[i], or i) and channel."""
    u = to_u8(img)
    if index is not None:
        u = u[np.asarray(index, dtype=np.int64)]
    v = u.reshape(u.shape[0], -1, 3).astype(np.uint64)
    out = np.empty((u.shape[0], 3, 4), dtype=np.uint64)
    out[:, :, 0] = v.sum(axis=1, dtype=np.uint64)
    out[:, :, 1] = (v * v).sum(axis=1, dtype=np.uint64)
    out[:, :, 2] = v.min(axis=1)
    out[:, :, 3] = v.max(axis=1)
    return out


def _f32(x):
    return np.float32(float(x))            # Fraction -> float64 (correctly rounded) -> float32


def combine_stats(per_image, pixels_per_image):
    """{"mean", "std", "min", "max"}: float32 [3, 1, 1] in [0, 1] over all the images of `per_image` (uint64 [n, 3, 4], stats_reference's or
    the device's), each of pixels_per_image pixels.  mean = S / (255 N), var = (N Q - S^2) / (255 N)^2, in integers and fractions."""
    p = np.asarray(per_image, dtype=np.uint64).reshape(-1, 3, 4)
    N = int(p.shape[0]) * int(pixels_per_image)
    if N < 1:
        raise ValueError("combine_stats: no pixels")
    out = {k: np.empty((3, 1, 1), dtype=np.float32) for k in ("mean", "std", "min", "max")}
    for c in range(3):
        S = sum(int(x) for x in p[:, c, 0])
        Q = sum(int(x) for x in p[:, c, 1])
        var = Fraction(N * Q - S * S, (255 * N) ** 2)
        out["mean"][c] = _f32(Fraction(S, 255 * N))
        out["std"][c] = np.float32(_sqrt_fraction(var))
        out["min"][c] = _f32(Fraction(min(int(x) for x in p[:, c, 2]), 255))
        out["max"][c] = _f32(Fraction(max(int(x) for x in p[:, c, 3]), 255))
    return out


def _sqrt_fraction(v):
    """sqrt of a non-negative Fraction, correctly rounded to float64: the integer square root of the value scaled by 4^k carries more than the
    53 bits a double keeps (and its remainder's sticky bit), so float() of the scaled root rounds once."""
    import math
    if v <= 0:
        return 0.0
    k = 128
    n = (v.numerator << (2 * k)) // v.denominator
    while n < (1 << 240):                  # tiny values: more bits
        k += 64
        n = (v.numerator << (2 * k)) // v.denominator
    r = math.isqrt(n)
    exact = r * r == n and (v.numerator << (2 * k)) % v.denominator == 0
    return float(Fraction(2 * r + (0 if exact else 1), 2 << k))


def identity_lut():
    """float32 [3, 256]: u / 255, the value the decoder's float format gives."""
    return np.tile(np.arange(256, dtype=np.float32) / np.float32(255), (3, 1))


def normalise_lut(mean, std):
    """float32 [3, 256]: (float32(u) / float32(255) - mean[c]) / std[c], every operation in float32."""
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((np.arange(256, dtype=np.float32) / np.float32(255))[None, :] - m) / s


def check_prep(src_shape, nlut, lut_index, box, src_index, out_hw):
    """The conditions avsim_image_prep puts on its host arrays (include/avsim.h); raises ValueError."""
    n, H, W = src_shape
    oh, ow = out_hw
    if not (1 <= oh <= 65535 and 1 <= ow <= 65535 and 1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError("image prep: a size outside 1..65535")
    for i, (x0, y0, flip) in enumerate(np.asarray(box, dtype=np.int64).reshape(-1, 3)):
        s = i if src_index is None else int(src_index[i])
        t = 0 if lut_index is None else int(lut_index[i])
        if not 0 <= s < n:
            raise ValueError(f"image prep: output {i}: source image out of range")
        if not 0 <= t < nlut:
            raise ValueError(f"image prep: output {i}: table out of range")
        if flip not in (0, 1):
            raise ValueError(f"image prep: output {i}: flip is 0 or 1")
        if x0 < 0 or y0 < 0 or x0 + ow > W or y0 + oh > H:
            raise ValueError(f"image prep: output {i}: the crop does not lie inside the source")


def prep_reference(img, lut, lut_index, box, out_hw, src_index=None):
    """float32 [nout, 3, oh, ow] (module docstring).  lut: float32 [nlut, 3, 256] (or [3, 256]); lut_index: int [nout] or None (table 0);
    box: int rows (x0, y0, flip); src_index: int [nout] or None (output i reads image i)."""
    u = to_u8(img)
    lut = np.asarray(lut, dtype=np.float32).reshape(-1, 3, 256)
    box = np.asarray(box, dtype=np.int64).reshape(-1, 3)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    check_prep(u.shape[:3], len(lut), lut_index, box, src_index, (oh, ow))
    out = np.empty((len(box), 3, oh, ow), dtype=np.float32)
    for i, (x0, y0, flip) in enumerate(box):
        crop = u[i if src_index is None else int(src_index[i]), y0:y0 + oh, x0:x0 + ow]
        if flip:
            crop = crop[:, ::-1]
        t = lut[0 if lut_index is None else int(lut_index[i])]
        for c in range(3):
            out[i, c] = t[c][crop[:, :, c]]
    return out


def center_box(src_hw, out_hw):
    """(x0, y0) of the centred crop."""
    return (int(src_hw[1]) - int(out_hw[1])) // 2, (int(src_hw[0]) - int(out_hw[0])) // 2


def chunk_index(ep_start, ep_len, frame, chunk):
    """(index int64 [B, chunk], is_pad bool [B, chunk]) of the chunks that start at the global frames `frame`: ep_start / ep_len are the
    first global frame and the length of every episode; for frame f at position t of an episode of length T starting at s,
    index[k] = s + min(t + k, T - 1) and is_pad[k] = t + k > T - 1."""
    ep_start = np.asarray(ep_start, dtype=np.int64)
    ep_len = np.asarray(ep_len, dtype=np.int64)
    f = np.asarray(frame, dtype=np.int64).reshape(-1)
    e = np.searchsorted(ep_start, f, side="right") - 1
    if len(f) and (f.min() < 0 or (f >= ep_start[e] + ep_len[e]).any()):
        raise IndexError("chunk_index: a frame outside the episodes")
    s, T = ep_start[e][:, None], ep_len[e][:, None]
    tk = (f[:, None] - s) + np.arange(int(chunk), dtype=np.int64)[None, :]
    return s + np.minimum(tk, T - 1), tk > T - 1


def history_index(ep_start, ep_len, frame, n_obs_steps):
    """(index int64 [B, K], is_pad bool [B, K]) of the observation histories that END at the global frames `frame` (K = n_obs_steps; slot
    K-1 is the frame itself): for frame f at position t of an episode starting at s, index[k] = s + max(t - (K-1) + k, 0) and is_pad[k] =
    t - (K-1) + k < 0 -- LeRobot's clamping of negative delta_timestamps, the counterpart of chunk_index."""
    ep_start = np.asarray(ep_start, dtype=np.int64)
    ep_len = np.asarray(ep_len, dtype=np.int64)
    f = np.asarray(frame, dtype=np.int64).reshape(-1)
    e = np.searchsorted(ep_start, f, side="right") - 1
    if len(f) and (f.min() < 0 or (f >= ep_start[e] + ep_len[e]).any()):
        raise IndexError("history_index: a frame outside the episodes")
    K = int(n_obs_steps)
    if K < 1:
        raise ValueError("history_index: n_obs_steps >= 1")
    s = ep_start[e][:, None]
    tk = (f[:, None] - s) - (K - 1) + np.arange(K, dtype=np.int64)[None, :]
    return s + np.maximum(tk, 0), tk < 0
