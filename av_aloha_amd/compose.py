"""Camera views put into one image: the specification of the device's composer (avsim_compose / avsim_compose_label,
csrc/avsim_compose.hip.h) in numpy, byte for byte, and the layouts of the two things it is used for -- the cameras of an episode side by
side (gym_guided_vision/scripts/visualize_episodes.py:67-98 save_videos, visualize_all_episodes.py:70-121) and a grid of the envs of a batch.

* `resize_reference`: a separable triangle filter whose support grows with the shrink factor (antialiased when shrinking, plain bilinear
  when enlarging) in Pillow's fixed-point scheme: per axis, in double, scale = n_in / n_out, fs = max(scale, 1), support = fs; for output
  coordinate i: center = (i + 0.5) scale, lo = max(0, (int)(center - support + 0.5)), hi = min(n_in, (int)(center + support + 0.5)), weights
  w_j = max(0, 1 - |(j + lo - center + 0.5) / fs|) divided by their sum, k_j = (int)(0.5 + w_j 2^22), and the output sample is
  clamp((2^21 + sum_j k_j p[lo + j]) >> 22, 0, 255).  The horizontal pass runs first, the vertical one on its u8 result; a pass whose sizes
  are equal is skipped.  It is `PIL.Image.resize(size, Image.BILINEAR)` to the byte (tests/test_compose_host.py), not cv2's INTER_LINEAR,
  which does not antialias (deviation).
* `compose_reference`, `label_reference`: what the two C entry points write.
* `layout_row`, `layout_grid`: rows of `places` for them.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22
MAX_RATIO = 16
GLYPHS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ :.-=/"
CELL_W, CELL_H = 6, 8


def axis_table(n_in, n_out):
    """-> (lo int [n_out], count int [n_out], k int32 [n_out, taps]): the integer coefficients of one axis."""
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    taps = 2 * math.ceil(support) + 1
    lo, cnt, k = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, taps), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        a = max(0, int(center - support + 0.5))
        b = min(n_in, int(center + support + 0.5))
        w = [max(0.0, 1.0 - abs((j + a - center + 0.5) / fs)) for j in range(b - a)]
        total = 0.0
        for x in w:
            total += x
        lo[i], cnt[i] = a, b - a
        for j, x in enumerate(w):
            k[i, j] = int(0.5 + (x / total if total != 0.0 else x) * (1 << PRECISION_BITS))
    return lo, cnt, k


def _resample_axis(a, n_out, axis):
    """u8 array, resampled along `axis` to n_out samples."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a
    lo, cnt, k = axis_table(n_in, n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for i in range(n_out):
        acc = np.tensordot(k[i, :cnt[i]].astype(np.int64), src[lo[i]:lo[i] + cnt[i]], axes=(0, 0))
        out[i] = np.clip(((1 << (PRECISION_BITS - 1)) + acc) >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_reference(img_u8_hwc, out_h, out_w):
    """u8 [H, W, C] (or [H, W]) -> u8 [out_h, out_w, C]; the input itself when the sizes are equal."""
    img = np.asarray(img_u8_hwc)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("resize_reference takes a u8 image [H, W, C]")
    out_h, out_w = int(out_h), int(out_w)
    if not (1 <= out_h <= 65535 and 1 <= out_w <= 65535):
        raise ValueError(f"resize_reference: size {out_h} x {out_w} outside 1..65535")
    if img.shape[0] > MAX_RATIO * out_h or img.shape[1] > MAX_RATIO * out_w:
        raise ValueError(f"resize_reference: {img.shape[0]} x {img.shape[1]} -> {out_h} x {out_w} shrinks by more than {MAX_RATIO}")
    return _resample_axis(_resample_axis(img, out_w, 1), out_h, 0)


def check_places(places, nsrc, src_h, src_w, nout, canvas_h, canvas_w):
    """The conditions avsim_compose puts on `places` (include/avsim.h); raises ValueError."""
    p = np.asarray(places, dtype=np.int64).reshape(-1, 6)
    for i, (o, s, x0, y0, w, h) in enumerate(p):
        if not (0 <= o < nout and 0 <= s < nsrc):
            raise ValueError(f"compose: place {i}: image index out of range")
        if not (1 <= w <= 65535 and 1 <= h <= 65535):
            raise ValueError(f"compose: place {i}: rectangle size outside 1..65535")
        if x0 < 0 or y0 < 0 or x0 + w > canvas_w or y0 + h > canvas_h:
            raise ValueError(f"compose: place {i}: rectangle outside the canvas")
        if src_w > MAX_RATIO * w or src_h > MAX_RATIO * h:
            raise ValueError(f"compose: place {i}: shrinks by more than {MAX_RATIO}")
    for o in np.unique(p[:, 0]):
        q = p[p[:, 0] == o]
        for a in range(len(q)):
            for b in range(a + 1, len(q)):
                if q[a, 2] < q[b, 2] + q[b, 4] and q[b, 2] < q[a, 2] + q[a, 4] and q[a, 3] < q[b, 3] + q[b, 5] and q[b, 3] < q[a, 3] + q[a, 5]:
                    raise ValueError(f"compose: two rectangles overlap on output image {int(o)}")
    return p


def compose_reference(canvas, src, places):
    """canvas u8 [nout, CH, CW, 3] (written in place and returned), src u8 [nsrc, H, W, 3], places rows (out image, src image, x0, y0, w, h):
    source image `src image` resampled to h x w is written to canvas[out image, y0:y0+h, x0:x0+w]."""
    canvas, src = np.asarray(canvas), np.asarray(src)
    if canvas.dtype != np.uint8 or src.dtype != np.uint8 or canvas.ndim != 4 or src.ndim != 4:
        raise ValueError("compose_reference takes u8 arrays [n, H, W, 3]")
    p = check_places(places, src.shape[0], src.shape[1], src.shape[2], canvas.shape[0], canvas.shape[1], canvas.shape[2])
    tables = {}          # the placements of a layout share a few sizes: resample a source image once per size
    for o, s, x0, y0, w, h in p:
        key = (int(s), int(h), int(w))
        if key not in tables:
            tables[key] = resize_reference(src[s], h, w)
        canvas[o, y0:y0 + h, x0:x0 + w] = tables[key]
    return canvas


_FONT = []


def font():
    """u8 [128, 7]: row r (top first) of character ch, bit 4 = the left pixel -- the library's table (avsim_compose_font; no device needed)."""
    if not _FONT:
        from . import _ffi
        rows = np.zeros((128, 7), np.uint8)
        _ffi.lib().avsim_compose_font(rows.ctypes.data)
        _FONT.append(rows)
    return _FONT[0]


def text_mask(text, scale=1):
    """bool [8 scale, 6 scale len(text)]: the glyph pixels of a line of text."""
    rows = font()
    m = np.zeros((CELL_H, CELL_W * len(text)), bool)
    for i, ch in enumerate(text):
        g = rows[ord(ch)] if ord(ch) < 128 else np.zeros(7, np.uint8)
        for r in range(7):
            for c in range(5):
                m[r, CELL_W * i + c] = (g[r] >> (4 - c)) & 1
    return np.repeat(np.repeat(m, scale, 0), scale, 1)


def label_reference(canvas, where, prefix, values, rgb):
    """canvas u8 [nout, CH, CW, 3] (written in place and returned); where rows (out image, x, y, scale); the text prefix + str(values[i]) (values
    None: the prefix alone) in the colour rgb = (r, g, b) or 0xRRGGBB; pixels outside the canvas are skipped."""
    canvas = np.asarray(canvas)
    if isinstance(rgb, (int, np.integer)):
        rgb = ((int(rgb) >> 16) & 255, (int(rgb) >> 8) & 255, int(rgb) & 255)
    if len(prefix) > 15:
        raise ValueError("label: the prefix has more than 15 characters")
    _, CH, CW, _ = canvas.shape
    for i, (o, x, y, scale) in enumerate(np.asarray(where, dtype=np.int64).reshape(-1, 4)):
        if not (0 <= o < canvas.shape[0] and 1 <= scale <= 64):
            raise ValueError(f"label {i}: image out of range or scale outside 1..64")
        m = text_mask(prefix + ("" if values is None else str(int(values[i]))), int(scale))
        ys, xs = np.nonzero(m)
        ys, xs = ys + y, xs + x
        ok = (ys >= 0) & (ys < CH) & (xs >= 0) & (xs < CW)
        canvas[o, ys[ok], xs[ok]] = rgb
    return canvas


def layout_row(sizes, height=None):
    """The reference's rule (visualize_episodes.py:71-88): sizes = [(h, w)] of the cameras in order -> (places rows (x0, y0, w, h), canvas_h,
    canvas_w): every camera at the smallest height (or `height`), new_w = int(min_h * w / h), the x offsets accumulate."""
    min_h = int(min(h for h, _ in sizes) if height is None else height)
    rows, x = [], 0
    for h, w in sizes:
        new_w = int(min_h * w / h)
        rows.append((x, 0, new_w, min_h))
        x += new_w
    return rows, min_h, x


def layout_grid(n, cell_h, cell_w, cols=None):
    """n cells in row-major order, cols = ceil(sqrt(n)) by default -> (places rows (x0, y0, w, h), canvas_h, canvas_w)."""
    n = int(n)
    cols = int(math.ceil(math.sqrt(n))) if cols is None else int(cols)
    if n < 1 or cols < 1:
        raise ValueError(f"layout_grid: n={n}, cols={cols}")
    nrows = (n + cols - 1) // cols
    return [((i % cols) * cell_w, (i // cols) * cell_h, cell_w, cell_h) for i in range(n)], nrows * cell_h, cols * cell_w
