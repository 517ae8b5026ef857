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
