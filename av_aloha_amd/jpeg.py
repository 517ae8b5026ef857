"""Baseline JPEG as libavsim's device encoder writes it (avsim_jpeg_encode, csrc/avsim_jpeg.hip.h), restated in numpy.

`encode_reference` is the specification of the device code: the two are equal byte for byte (tests/test_gpu_jpeg.py), because every
step is integer arithmetic.  The stream: baseline sequential (SOF0), 8 bit, JFIF 1.1, Y Cb Cr 4:2:0 (an MCU is 16 x 16 pixels, blocks
Y00 Y01 Y10 Y11 Cb Cr), the four "typical" Huffman tables of ITU-T T.81 Annex K in every frame, one restart interval per MCU row.
It is slow (a Python loop per block) and meant for tests and for single frames."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K tables K.1 / K.2: quantiser steps at quality 50, natural (row-major) order
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# T.81 Annex K tables K.3 - K.6: (codes of each length 1..16, symbols in code order)
_DC_SYMBOLS = list(range(12))
HUFF_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _DC_SYMBOLS)
HUFF_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _DC_SYMBOLS)
HUFF_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
# DHT order of the stream: (Tc << 4 | Th, table)
HUFF_TABLES = ((0x00, HUFF_DC_LUMA), (0x10, HUFF_AC_LUMA), (0x01, HUFF_DC_CHROMA), (0x11, HUFF_AC_CHROMA))

# forward DCT in 13-bit fixed point: DCT_MATRIX[k][n] = round(8192 c(k)/2 cos((2n+1) k pi / 16)), c(0) = 1/sqrt 2
DCT_MATRIX = np.rint(8192 * np.array([[(np.sqrt(0.5) if k == 0 else 1.0) * 0.5 * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)]
                                      for k in range(8)])).astype(np.int64)

# the longest code of a block: 63 AC coefficients of 16 + 10 bits and a DC difference of 11 + 11 bits, in bytes; every byte stuffed
BLOCK_BYTES_MAX = (63 * 26 + 22 + 7) // 8
HEADER_BYTES = 629


def quant_table(base, quality):
    """libjpeg's quality rule on an Annex K table (natural order)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {quality} outside 1..100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255)


def huffman_codes(bits, symbols):
    """{symbol: (code, length)} of a DHT table (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _check_size(height, width):
    if not (1 <= height <= 65535 and 1 <= width <= 65535):
        raise ValueError(f"image size {height} x {width} outside 1..65535")


def header(height, width, quality):
    """Everything in front of the entropy-coded data: SOI APP0 DQT DQT SOF0 DHT x 4 DRI SOS.  Depends on (H, W, quality) only."""
    _check_size(height, width)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, base in ((0, QUANT_LUMA), (1, QUANT_CHROMA)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(quant_table(base, quality)[ZIGZAG].astype(np.uint8))
    out += b"\xff\xc0\x00\x11\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc, (bits, symbols) in HUFF_TABLES:
        out += b"\xff\xc4" + (19 + len(symbols)).to_bytes(2, "big") + bytes([tc]) + bytes(bits) + bytes(symbols)
    out += b"\xff\xdd\x00\x04" + ((width + 15) // 16).to_bytes(2, "big")
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def bound(height, width):
    """Worst-case stream length of an H x W image at any quality (avsim_jpeg_bound): header, every coefficient at its longest code with
    every byte stuffed, the restart markers, EOI."""
    _check_size(height, width)
    mh, mw = (height + 15) // 16, (width + 15) // 16
    return HEADER_BYTES + mh * mw * 6 * 2 * BLOCK_BYTES_MAX + 2 * (mh - 1) + 2


def _fdct_quant(blocks, q):
    """blocks [..., 8, 8] level-shifted samples, q[64] in natural order -> quantised coefficients [..., 64] in natural order."""
    t = (np.einsum("kn,...rn->...rk", DCT_MATRIX, blocks) + 1024) >> 11          # rows
    s = np.einsum("kr,...rc->...kc", DCT_MATRIX, t)                             # columns
    s = s.reshape(s.shape[:-2] + (64,))
    den = q.astype(np.int64) << 15
    return np.sign(s) * ((np.abs(s) + (den >> 1)) // den)                        # round half away from zero


def _block_symbols(z, pred, dc, ac, acc):
    """Append the (code, length) pairs of one block (zigzag order) to acc; returns the block's DC."""
    diff = int(z[0]) - pred
    n = abs(diff).bit_length()
    acc.append(dc[n])
    if n:
        acc.append(((diff if diff > 0 else diff - 1) & ((1 << n) - 1), n))
    last = 0
    for k in np.nonzero(z[1:])[0]:
        k = int(k) + 1
        run = k - last - 1
        last = k
        while run > 15:
            acc.append(ac[0xF0])
            run -= 16
        v = int(z[k])
        n = abs(v).bit_length()
        acc.append(ac[(run << 4) | n])
        acc.append(((v if v > 0 else v - 1) & ((1 << n) - 1), n))
    if last != 63:
        acc.append(ac[0])
    return int(z[0])


def encode_reference(img, quality=90):
    """u8 [H, W, 3] RGB -> the JPEG stream (bytes)."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("encode_reference takes a u8 [H, W, 3] image")
    H, W, _ = img.shape
    out = bytearray(header(H, W, quality))
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    p = np.pad(img, ((0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = np.clip((19595 * R + 38470 * G + 7471 * B + 32768) >> 16, 0, 255)
    Cb = np.clip(((-11059 * R - 21709 * G + 32768 * B + 32768) >> 16) + 128, 0, 255)
    Cr = np.clip(((32768 * R - 27439 * G - 5329 * B + 32768) >> 16) + 128, 0, 255)

    def sub(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2

    def blocks(a):
        return a.reshape(a.shape[0] // 8, 8, a.shape[1] // 8, 8).transpose(0, 2, 1, 3) - 128

    ql, qc = quant_table(QUANT_LUMA, quality), quant_table(QUANT_CHROMA, quality)
    cy = _fdct_quant(blocks(Y), ql)[..., ZIGZAG]
    cb = _fdct_quant(blocks(sub(Cb)), qc)[..., ZIGZAG]
    cr = _fdct_quant(blocks(sub(Cr)), qc)[..., ZIGZAG]
    dc = [huffman_codes(*HUFF_DC_LUMA), huffman_codes(*HUFF_DC_CHROMA)]
    ac = [huffman_codes(*HUFF_AC_LUMA), huffman_codes(*HUFF_AC_CHROMA)]
    for r in range(Hp // 16):
        acc = []
        py = pb = pr = 0
        for m in range(Wp // 16):
            for yy, xx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                py = _block_symbols(cy[2 * r + yy, 2 * m + xx], py, dc[0], ac[0], acc)
            pb = _block_symbols(cb[r, m], pb, dc[1], ac[1], acc)
            pr = _block_symbols(cr[r, m], pr, dc[1], ac[1], acc)
        # the interval's bits, most significant first, in pieces of at most 4096 symbols (one huge integer would cost quadratic time)
        data = bytearray()
        v = n = 0
        for code, length in acc:
            v = (v << length) | code
            n += length
            if n >= 32768:
                keep = n & 7
                data += (v >> keep).to_bytes(n >> 3, "big")
                v &= (1 << keep) - 1
                n = keep
        pad = -n % 8
        v = (v << pad) | ((1 << pad) - 1)
        data += v.to_bytes((n + pad) // 8, "big")
        if r:
            out += bytes([0xFF, 0xD0 + ((r - 1) & 7)])
        out += data.replace(b"\xff", b"\xff\x00")
    out += b"\xff\xd9"
    return bytes(out)


# ---- decoding (avsim_jpeg_decode, csrc/avsim_jpeg.hip.h: k_jpeg_index, k_jpeg_entropy, k_jpeg_reconstruct) ---------------------------------
STATUS_HEADER, STATUS_STRUCTURE, STATUS_ENTROPY = 1, 2, 4
_DQT_PAYLOADS = ((25, 89), (94, 158))           # the 2 x 64 quantiser bytes (zigzag order) inside header()
_SOF_SIZE = 163                                 # height, width: two big-endian uint16


class JpegError(ValueError):
    """A stream decode_reference / parse does not read; `status` is the bit avsim_jpeg_decode reports for it."""

    def __init__(self, status, msg):
        super().__init__(msg)
        self.status = status


def stream_size(stream):
    """(height, width) of a stream of this encoder: the cheap form of parse (the header is compared, the entropy data is not walked)."""
    s = bytes(stream[:HEADER_BYTES])
    if len(stream) < HEADER_BYTES + 2:
        raise JpegError(STATUS_STRUCTURE, f"{len(stream)} bytes: shorter than the header and EOI")
    H, W = int.from_bytes(s[_SOF_SIZE:_SOF_SIZE + 2], "big"), int.from_bytes(s[_SOF_SIZE + 2:_SOF_SIZE + 4], "big")
    if H < 1 or W < 1:
        raise JpegError(STATUS_HEADER, "not this encoder's header")
    want = header(H, W, 50)
    (a0, a1), (b0, b1) = _DQT_PAYLOADS
    if s[:a0] != want[:a0] or s[a1:b0] != want[a1:b0] or s[b1:] != want[b1:]:
        raise JpegError(STATUS_HEADER, "not this encoder's header")
    return H, W


def parse(stream):
    """{"height", "width", "quant": [luma[64], chroma[64]] (natural order, read from the stream), "intervals": [(begin, end)] byte ranges of
    the restart intervals}.  Raises JpegError (a ValueError) unless the stream has encode_reference's structure: header(H, W, q) byte for
    byte apart from the DQT payloads, exactly ceil(H / 16) intervals separated by RST0..7 in order, EOI at the end."""
    stream = bytes(stream)
    H, W = stream_size(stream)
    inv = np.argsort(ZIGZAG)
    quant = [np.frombuffer(stream[a:b], np.uint8).astype(np.int64)[inv] for a, b in _DQT_PAYLOADS]
    n, mh = len(stream), (H + 15) // 16
    if stream[n - 2:] != b"\xff\xd9":
        raise JpegError(STATUS_STRUCTURE, "no EOI at the end")
    a = np.frombuffer(stream, np.uint8)
    marks = HEADER_BYTES + np.nonzero((a[HEADER_BYTES:n - 2] == 0xFF) & (a[HEADER_BYTES + 1:n - 1] != 0))[0]      # stuffing leaves FF 00 only
    code = a[marks + 1].astype(np.int64) - 0xD0
    if len(marks) != mh - 1 or not np.array_equal(code, np.arange(mh - 1) & 7):
        raise JpegError(STATUS_STRUCTURE, f"{len(marks)} markers in the entropy-coded data, not RST0..7 in order {mh - 1} times")
    edges = [HEADER_BYTES - 2] + [int(m) for m in marks] + [n - 2]
    return {"height": H, "width": W, "quant": quant, "intervals": [(edges[r] + 2, edges[r + 1]) for r in range(mh)]}


def _decode_luts():
    """Per table of HUFF_TABLES: uint32[65536], (symbol << 8 | length) of the code the next 16 bits start with, 0 where none does."""
    out = []
    for _, (bits, symbols) in HUFF_TABLES:
        lut = np.zeros(65536, np.uint32)
        for sym, (code, length) in huffman_codes(bits, symbols).items():
            lut[code << (16 - length):(code + 1) << (16 - length)] = (sym << 8) | length
        out.append(lut.tolist())
    return out


_LUTS = []


def decode_interval(data, nblocks_mcu):
    """The quantised coefficients int64 [nblocks_mcu, 6, 64] (natural order) of one restart interval's bytes (still stuffed)."""
    if not _LUTS:
        _LUTS.extend(_decode_luts())
    dc_l, ac_l, dc_c, ac_c = _LUTS
    raw = bytes(data).replace(b"\xff\x00", b"\xff")
    total = 8 * len(raw)
    big = int.from_bytes(raw, "big") if raw else 0
    pos = 0                                      # bits consumed
    zz = ZIGZAG.tolist()
    out = np.zeros((nblocks_mcu, 6, 64), np.int64)
    pred = [0, 0, 0]

    def peek16():
        left = total - pos
        return (big >> (left - 16)) & 0xFFFF if left >= 16 else (big << (16 - left)) & 0xFFFF

    def symbol(lut):
        nonlocal pos
        e = lut[peek16()]
        if not e:
            raise JpegError(STATUS_ENTROPY, "a code that is not in the table")
        if pos + (e & 255) > total:
            raise JpegError(STATUS_ENTROPY, "the interval's bytes run out")
        pos += e & 255
        return e >> 8

    def amplitude(n):
        nonlocal pos
        if n == 0:
            return 0
        if pos + n > total:
            raise JpegError(STATUS_ENTROPY, "the interval's bytes run out")
        v = (big >> (total - pos - n)) & ((1 << n) - 1)
        pos += n
        return v if v >= 1 << (n - 1) else v - (1 << n) + 1

    for m in range(nblocks_mcu):
        for j in range(6):
            comp = 0 if j < 4 else j - 3
            n = symbol(dc_l if comp == 0 else dc_c)
            if n > 11:
                raise JpegError(STATUS_ENTROPY, "a DC size above 11")
            pred[comp] += amplitude(n)
            out[m, j, 0] = min(max(pred[comp], -32768), 32767)      # (the staging area is int16; no stream of the encoder comes near)
            ac, k = (ac_l if comp == 0 else ac_c), 1
            while k < 64:
                rs = symbol(ac)
                if rs == 0:
                    break
                run, n = rs >> 4, rs & 15
                if n > 10:
                    raise JpegError(STATUS_ENTROPY, "an AC size above 10")
                k += run
                if n == 0:                       # ZRL: sixteen zeros (the table has no other symbol of size 0)
                    k += 1
                    if k > 63:
                        raise JpegError(STATUS_ENTROPY, "a coefficient index past 63")
                    continue
                if k > 63:
                    raise JpegError(STATUS_ENTROPY, "a coefficient index past 63")
                out[m, j, zz[k]] = amplitude(n)
                k += 1
    left = total - pos
    if left >= 8 or (big & ((1 << left) - 1)) != (1 << left) - 1:
        raise JpegError(STATUS_ENTROPY, "whole bytes left over or a pad bit that is not 1 at the interval's end")
    return out


def decode_coefficients(stream):
    """parse + entropy decode: (info, Y [2 mh, 2 mw, 64], Cb [mh, mw, 64], Cr [mh, mw, 64]) quantised coefficients, natural order."""
    info = parse(stream)
    H, W = info["height"], info["width"]
    mh, mw = (H + 15) // 16, (W + 15) // 16
    cy, cb, cr = np.zeros((2 * mh, 2 * mw, 64), np.int64), np.zeros((mh, mw, 64), np.int64), np.zeros((mh, mw, 64), np.int64)
    for r, (a, b) in enumerate(info["intervals"]):
        c = decode_interval(stream[a:b], mw)
        cy[2 * r:2 * r + 2] = c[:, :4].reshape(mw, 2, 2, 64).transpose(1, 0, 2, 3).reshape(2, 2 * mw, 64)
        cb[r], cr[r] = c[:, 4], c[:, 5]
    return info, cy, cb, cr


def _idct(coef, q):
    """coef [by, bx, 64] quantised, q[64] -> u8-valued samples [8 by, 8 bx] (int64): dequantise, clamp, columns, rows, + 128, clamp."""
    F = np.clip(coef * q, -2048, 2047).reshape(coef.shape[:2] + (8, 8))                       # [.., k, l]
    t = (np.einsum("kr,...kl->...rl", DCT_MATRIX, F) + 1024) >> 11                            # columns
    p = (np.einsum("lc,...rl->...rc", DCT_MATRIX, t) + 16384) >> 15                           # rows
    p = np.clip(p + 128, 0, 255)
    return p.transpose(0, 2, 1, 3).reshape(coef.shape[0] * 8, coef.shape[1] * 8)


def dequantised_peak(stream):
    """max |coef * q| over the stream's coefficients: what the dequantiser's clamp to [-2048, 2047] would act on."""
    info, cy, cb, cr = decode_coefficients(stream)
    ql, qc = info["quant"]
    return int(max(np.abs(cy * ql).max(), np.abs(cb * qc).max(), np.abs(cr * qc).max()))


def _upsample_triangle(c, H, W):
    """libjpeg's h2v2 "fancy" filter on the chroma plane cropped to ceil(H/2) x ceil(W/2), edge samples replicated -> [H, W]."""
    ch, cw = (H + 1) // 2, (W + 1) // 2
    c = c[:ch, :cw]
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * ch, cw), np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    o = np.empty((2 * ch, 2 * cw), np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
    return o[:H, :W]


def decode_reference(stream, upsample="replicate"):
    """A stream of encode_reference (or of the device encoder) -> u8 [H, W, 3] RGB.  The specification of avsim_jpeg_decode: integer
    arithmetic throughout, equal to the device's output byte for byte (tests/test_gpu_jpeg_decode.py).  upsample "replicate": a chroma
    sample covers its 2 x 2 pixels (the inverse of the encoder's box filter); "triangle": libjpeg's default filter, what cv2 / Pillow show.
    Raises JpegError for a stream that is not this encoder's (parse) or whose entropy-coded data is broken."""
    if upsample not in ("replicate", "triangle"):
        raise ValueError(f"upsample {upsample!r}: 'replicate' or 'triangle'")
    info, cy, cb, cr = decode_coefficients(stream)
    H, W = info["height"], info["width"]
    ql, qc = info["quant"]
    Y = _idct(cy, ql)[:H, :W]
    Cb, Cr = _idct(cb, qc), _idct(cr, qc)
    if upsample == "replicate":
        Cb, Cr = (np.repeat(np.repeat(c, 2, 0), 2, 1)[:H, :W] for c in (Cb, Cr))
    else:
        Cb, Cr = _upsample_triangle(Cb, H, W), _upsample_triangle(Cr, H, W)
    Cb, Cr = Cb - 128, Cr - 128
    R = Y + ((91881 * Cr + 32768) >> 16)
    G = Y - ((22554 * Cb + 46802 * Cr + 32768) >> 16)
    B = Y + ((116130 * Cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)
