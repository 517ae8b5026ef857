"""Motion-JPEG in an AVI container, written and read with `struct` alone (no cv2 / imageio / av where this runs).

    w = AviWriter("rollout_0.avi", 640, 480, fps=50)
    for stream in jpeg_streams:          # bytes of one complete JPEG each (av_aloha_amd/jpeg.py, BatchedSim.encode_jpeg, VecEnv.encode_jpeg)
        w.add(stream)
    w.close()
    info, frames = read_avi("rollout_0.avi")

Layout (RIFF `AVI `, the AVI 1.0 structures every player reads): LIST `hdrl` { `avih` main header, LIST `strl` { `strh` with type `vids` and
handler `MJPG`, `strf` = BITMAPINFOHEADER with compression `MJPG`, 24 bit } }, LIST `movi` of `00dc` chunks (one frame each, padded to even
length), `idx1` with one key-frame entry per chunk.  The file is written to `<path>.part` and renamed when it is complete, so a reader
never sees half a video; sizes and the frame count are patched into the headers at close().  A file stays below 4 GiB (RIFF's 32-bit sizes)."""
from __future__ import annotations

import os
import struct

_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10


class AviWriter:
    def __init__(self, path, width, height, fps=50):
        if not (0 < int(width) < 65536 and 0 < int(height) < 65536):
            raise ValueError(f"AviWriter: frame size {width} x {height}")
        if not fps > 0:
            raise ValueError(f"AviWriter: fps {fps}")
        self.path, self.width, self.height, self.fps = str(path), int(width), int(height), float(fps)
        # frame rate as rate / scale with three decimals (50 -> 50000 / 1000)
        self._scale, self._rate = 1000, int(round(self.fps * 1000))
        self._part = self.path + ".part"
        self._f = open(self._part, "wb")
        self._index = []          # (offset from the 'movi' fourcc, length) of every frame chunk
        self._max = 0
        self._f.write(self._headers(0, 0, 0))
        self._movi = self._f.tell() - 4        # position of the 'movi' fourcc
        self._bytes = 4

    def _headers(self, frames, movi_size, riff_size):
        usec = int(round(1e6 / self.fps))
        avih = struct.pack("<14I", usec, int(self._max * self.fps), 0, _AVIF_HASINDEX, frames, 0, 1, self._max, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate, 0, frames, self._max, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        chunk = lambda tag, data: tag + struct.pack("<I", len(data)) + data
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + chunk(b"avih", avih) + strl
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_size) + b"movi"

    def add(self, jpeg_bytes):
        """One frame: a complete JPEG stream (SOI ... EOI)."""
        data = bytes(jpeg_bytes)
        if data[:2] != b"\xff\xd8":
            raise ValueError("AviWriter.add: not a JPEG stream")
        if self._f.tell() + len(data) + 16 * (len(self._index) + 2) + 64 >= 1 << 32:
            raise ValueError("AviWriter: the file would pass 4 GiB")
        self._index.append((self._bytes, len(data)))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1))
        self._bytes += 8 + len(data) + (len(data) & 1)
        self._max = max(self._max, len(data))

    def close(self):
        if self._f is None:
            return
        f = self._f
        idx = b"".join(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, n) for off, n in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        size = f.tell()
        f.seek(0)
        f.write(self._headers(len(self._index), self._bytes, size - 8))
        assert f.tell() == self._movi + 4
        f.close()
        self._f = None
        os.replace(self._part, self.path)

    def abort(self):
        """Drop the unfinished file."""
        if self._f is not None:
            self._f.close()
            self._f = None
            if os.path.exists(self._part):
                os.remove(self._part)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()


def _chunks(buf, start, end):
    pos = start
    while pos + 8 <= end:
        tag, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        yield tag, pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """-> (info, frames): info = {"width", "height", "fps", "frames", "codec"}, frames = the `00dc` chunks' bytes in file order.  Reads
    what AviWriter writes and other AVI 1.0 files with one video stream; the index is checked against the chunks when present."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    end = min(len(buf), 8 + struct.unpack_from("<I", buf, 4)[0])
    info, frames, offsets, index, movi = {}, [], [], None, None
    for tag, pos, size in _chunks(buf, 12, end):
        if tag == b"LIST" and buf[pos:pos + 4] == b"hdrl":
            for t2, p2, s2 in _chunks(buf, pos + 4, pos + size):
                if t2 == b"avih":
                    a = struct.unpack_from("<14I", buf, p2)
                    info.update(frames=a[4], width=a[8], height=a[9])
                elif t2 == b"LIST" and buf[p2:p2 + 4] == b"strl":
                    for t3, p3, s3 in _chunks(buf, p2 + 4, p2 + s2):
                        if t3 == b"strh" and buf[p3:p3 + 4] == b"vids":
                            scale, rate = struct.unpack_from("<II", buf, p3 + 20)
                            info.update(fps=rate / scale, codec=buf[p3 + 4:p3 + 8].decode("latin1"))
                        elif t3 == b"strf":
                            w, h = struct.unpack_from("<ii", buf, p3 + 4)
                            info.update(width=w, height=abs(h))
        elif tag == b"LIST" and buf[pos:pos + 4] == b"movi":
            movi = pos
            for t2, p2, s2 in _chunks(buf, pos + 4, pos + size):
                if t2[2:] in (b"dc", b"db"):
                    frames.append(buf[p2:p2 + s2])
                    offsets.append((p2 - 8 - movi, s2))
        elif tag == b"idx1":
            index = [struct.unpack_from("<4sIII", buf, pos + 16 * i) for i in range(size // 16)]
    if movi is None or "width" not in info:
        raise ValueError(f"{path}: no header or no movi list")
    if index is not None:
        got = [(off, n) for _, _, off, n in index]
        if got != offsets:
            raise ValueError(f"{path}: idx1 does not describe the movi chunks")
    if info.get("frames") != len(frames):
        raise ValueError(f"{path}: header says {info.get('frames')} frames, the file holds {len(frames)}")
    return info, frames
