"""The device image calls of libavsim (JPEG encode and decode, compose and label, image statistics, prep, jitter, augment and resize; include/avsim.h) from
Python: what BatchedSim's numpy methods and the torch methods share, the torch methods themselves (DeviceImageOps, which VecEnv inherits)
and DeviceImages, the same methods for a caller that has no env (a data set, a video tool)."""
import numpy as np

from . import _ffi


def check_call(handle, rc):
    """The status of an image entry point: AVSIM_EINVAL (-1) -- the library refused the arguments and launched nothing -- is a ValueError
    with its message, every other failure Handle.check's AvsimError."""
    if rc == -1:
        raise ValueError(handle.L.avsim_last_error(handle.h).decode())
    handle.check(rc)


_DTYPE_NAME = {}


def layout(a):
    """(fmt, n, H, W) of an image batch, numpy or torch: fmt 0 = uint8 [n, H, W, 3], 1 = float32 [n, 3, H, W]; ValueError for anything else."""
    dtype = _DTYPE_NAME.get(a.dtype) or _DTYPE_NAME.setdefault(a.dtype, str(a.dtype).rsplit(".", 1)[-1])      # (str() of a dtype per call is slow)
    if a.ndim == 4 and dtype == "uint8" and a.shape[3] == 3:
        return 0, int(a.shape[0]), int(a.shape[1]), int(a.shape[2])
    if a.ndim == 4 and dtype == "float32" and a.shape[1] == 3:
        return 1, int(a.shape[0]), int(a.shape[2]), int(a.shape[3])
    raise ValueError("compose: images are uint8 [n, H, W, 3] or float32 [n, 3, H, W]")


def default_stride(L, H, W, divisor):
    """Bytes reserved per JPEG stream of an H x W image when the caller says nothing: the raw frame's over `divisor` in whole 4 KB, never
    more than the worst case (avsim_jpeg_bound)."""
    return int(min(L.avsim_jpeg_bound(H, W), (H * W * 3 // divisor + 4095) // 4096 * 4096))


def camera_ids(manifest, cameras):
    """int32 ids of cameras given by name (the manifest's camera table) or by index."""
    names = manifest["camera_names"]
    return np.array([names.index(c) if isinstance(c, str) else int(c) for c in cameras], dtype=np.int32)


class DeviceImageOps:
    """The image calls on torch tensors, for the owner of a device-I/O handle: self.h (_ffi.Handle), self.L, self.device, self.torch,
    self._stream = None, and -- decode_jpeg's defaults -- self.obs_format, self.observation_height and self.observation_width.  Every call
    runs on torch's current stream (re-bound when it changes) and none synchronises it; close() waits for it and gives the handle back."""

    def _bind_stream(self):
        s = self.torch.cuda.current_stream(self.device)
        if self._stream is None or s.cuda_stream != self._stream.cuda_stream:
            self.h.check(self.L.avsim_set_stream(self.h.h, s.cuda_stream))
            self._stream = s

    def close(self):
        if getattr(self, "h", None) is not None:
            self.h.check(self.L.avsim_sync(self.h.h))
            self.h.close()
            self.h = None

    def _canvas_of(self, t):
        assert isinstance(t, self.torch.Tensor) and t.device == self.device and t.is_contiguous() and t.ndim == 4, "a contiguous 4-D tensor on the env's device"
        fmt, n, H, W = layout(t)
        return fmt, (n, H, W)

    def decode_jpeg(self, buf, lengths, height=None, width=None, upsample="replicate", fmt=None, out=None, status=None):
        """The inverse of encode_jpeg on the device (avsim_jpeg_decode): buf uint8 [n, stride] and lengths int32 [n] as encode_jpeg
        returns them -> (images, status int32 [n]).  height / width default to the observation size, fmt to the env's observation format:
        "lerobot" float32 [n, 3, H, W] in [0, 1], "gym" uint8 [n, H, W, 3].  The pixels are av_aloha_amd.jpeg.decode_reference's;
        status[i] != 0 flags a stream that is not this encoder's (avsim.h), whose image is unspecified.  out / status: buffers to write
        into.  Does not synchronise -- so it does not raise for a flagged stream either: read `status` when the host next waits."""
        torch = self.torch
        self._bind_stream()
        if upsample not in ("replicate", "triangle"):
            raise ValueError(f"upsample {upsample!r}: 'replicate' or 'triangle'")
        fmt = self.obs_format if fmt is None else fmt
        if fmt not in ("lerobot", "gym"):
            raise ValueError(f"fmt {fmt!r}: 'lerobot' or 'gym'")
        H = self.observation_height if height is None else int(height)
        W = self.observation_width if width is None else int(width)
        if H is None or W is None:
            raise ValueError("decode_jpeg: give height and width (there is no observation size to default to)")
        assert buf.dtype == torch.uint8 and buf.device == self.device and buf.ndim == 2 and buf.is_contiguous()
        n = int(buf.shape[0])
        assert lengths.dtype == torch.int32 and lengths.device == self.device and tuple(lengths.shape) == (n,) and lengths.is_contiguous()
        shape, dtype = ((n, 3, H, W), torch.float32) if fmt == "lerobot" else ((n, H, W, 3), torch.uint8)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        assert out.dtype == dtype and out.device == self.device and tuple(out.shape) == shape and out.is_contiguous()
        assert status.dtype == torch.int32 and status.device == self.device and tuple(status.shape) == (n,) and status.is_contiguous()
        self.h.check(self.L.avsim_jpeg_decode(self.h.h, buf.data_ptr(), int(buf.shape[1]), lengths.data_ptr(), None, n, H, W,
                                              1 if fmt == "lerobot" else 0, 1 if upsample == "triangle" else 0, out.data_ptr(), status.data_ptr()))
        return out, status

    def encode_images(self, images, quality=90, out=None, out_len=None):
        """JPEG streams of any image batch on the env's device -- uint8 [n, H, W, 3] or float32 [n, 3, H, W], a compose() canvas for one --
        through avsim_jpeg_encode: -> (out uint8 [n, stride], out_len int32 [n]) as encode_jpeg returns them.  Does not synchronise."""
        self._bind_stream()
        fmt, (n, H, W) = self._canvas_of(images)
        return self._encode(images, fmt, None, n, H, W, quality, out, out_len)

    def _encode(self, img, fmt, index, n, H, W, quality, out, out_len):
        torch = self.torch
        if out is None:
            out = torch.empty((n, default_stride(self.L, H, W, 2)), dtype=torch.uint8, device=self.device)
        if out_len is None:
            out_len = torch.empty(n, dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and out.device == self.device and out.ndim == 2 and out.shape[0] == n and out.is_contiguous()
        assert out_len.dtype == torch.int32 and out_len.device == self.device and tuple(out_len.shape) == (n,) and out_len.is_contiguous()
        self.h.check(self.L.avsim_jpeg_encode(self.h.h, img.data_ptr(), fmt, _ffi.ptr(index), n, H, W, int(quality), out.data_ptr(), int(out.shape[1]), out_len.data_ptr()))
        return out, out_len

    def compose(self, src, places, out=None, canvas_hw=None, nout=None, clear=None, fmt=None):
        """Images resampled into rectangles of a canvas (avsim_compose; av_aloha_amd.compose.compose_reference's pixels).  src: a tensor on
        the env's device, uint8 [n, H, W, 3] or float32 [n, 3, H, W] -- an observation of this env, a decode_jpeg result --; places: HOST int
        rows (out image, src image, x0, y0, w, h), checked on the host (ValueError).  out: the canvas tensor (either format), written in
        place; None: one of canvas_hw = (CH, CW) and nout images is allocated in format fmt ("gym" u8 HWC, the default, or "lerobot" float32
        CHW) and cleared.  clear: 0xRRGGBB to fill the canvas with first.  Does not synchronise."""
        torch = self.torch
        self._bind_stream()
        p = np.ascontiguousarray(places, dtype=np.int32).reshape(-1, 6)
        sf, (n, H, W) = self._canvas_of(src)
        if out is None:
            if canvas_hw is None:
                raise ValueError("compose: give a canvas (out=...) or its size (canvas_hw=...)")
            if fmt not in (None, "gym", "lerobot"):
                raise ValueError(f"fmt {fmt!r}: 'lerobot' or 'gym'")
            nout = int(p[:, 0].max()) + 1 if nout is None and len(p) else int(nout or 1)
            CH, CW = int(canvas_hw[0]), int(canvas_hw[1])
            out = torch.empty((nout, 3, CH, CW), dtype=torch.float32, device=self.device) if fmt == "lerobot" else \
                torch.empty((nout, CH, CW, 3), dtype=torch.uint8, device=self.device)
            clear = 0 if clear is None else clear
        df, (no, CH, CW) = self._canvas_of(out)
        check_call(self.h, self.L.avsim_compose(self.h.h, src.data_ptr(), sf, n, H, W, out.data_ptr(), df, no, CH, CW, p.ctypes.data, len(p),
                                                0 if clear is None else 1, int(clear or 0) & 0xFFFFFF))
        return out

    def compose_label(self, canvas, where, prefix="", values=None, rgb=0xFFFFFF):
        """prefix + the decimal digits of values[i] painted at where[i] = (out image, x, y, scale) (avsim_compose_label;
        av_aloha_amd.compose.label_reference's pixels).  values: an int64 tensor [len(where)] on the env's device -- info["episode_id"], read by
        the kernel --, or None: the prefix alone; where: HOST rows.  Writes the canvas in place; does not synchronise."""
        torch = self.torch
        self._bind_stream()
        df, (no, CH, CW) = self._canvas_of(canvas)
        w = np.ascontiguousarray(where, dtype=np.int32).reshape(-1, 4)
        if values is not None:
            assert isinstance(values, torch.Tensor) and values.dtype == torch.int64 and values.device == self.device and tuple(values.shape) == (len(w),) \
                and values.is_contiguous(), "compose_label(values=...): a contiguous int64 tensor on the env's device, one value per label"
        check_call(self.h, self.L.avsim_compose_label(self.h.h, canvas.data_ptr(), df, no, CH, CW, w.ctypes.data, len(w), prefix.encode("ascii", "replace"),
                                                      _ffi.ptr(values), int(rgb) & 0xFFFFFF))
        return canvas

    def image_stats(self, img, index=None, out=None):
        """(sum, sum of squares, min, max) of the u8 values per image and channel (avsim_image_stats; av_aloha_amd.imgprep.stats_reference's
        integers): img a tensor on the env's device, uint8 [n, H, W, 3] or float32 [n, 3, H, W]; index: an int32 tensor there, the images to
        reduce in this order (values outside [0, n) are clamped), None: all.  -> int64 [m, 3, 4] on the device (the values are below 2^63).
        Does not synchronise."""
        torch = self.torch
        self._bind_stream()
        sf, (n, H, W) = self._canvas_of(img)
        if index is not None:
            assert isinstance(index, torch.Tensor) and index.dtype == torch.int32 and index.device == self.device and index.ndim == 1, \
                "image_stats(index=...): an int32 index tensor on the env's device"
            index = index.clamp(0, n - 1).contiguous()
        m = n if index is None else int(index.shape[0])
        if out is None:
            out = torch.empty((m, 3, 4), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and out.device == self.device and tuple(out.shape) == (m, 3, 4) and out.is_contiguous()
        check_call(self.h, self.L.avsim_image_stats(self.h.h, img.data_ptr(), sf, _ffi.ptr(index), m, H, W, out.data_ptr()))
        return out

    def prep_images(self, img, lut, box, out_hw, lut_index=None, src_index=None, out=None):
        """Crops of img, mirrored where box says so, every channel through a table (avsim_image_prep; av_aloha_amd.imgprep.prep_reference's
        bits).  img: a tensor on the env's device, uint8 [n, H, W, 3] or float32 [n, 3, H, W] -- an observation, a decode_jpeg result --; lut:
        a float32 tensor [nlut, 3, 256] (or [3, 256]) there; box: HOST int rows (x0, y0, flip), one per output; lut_index / src_index: HOST
        int arrays, the table / the source image of every output (None: table 0 / image i), all checked on the host (ValueError) and copied
        by the library before the call returns.  -> float32 [nout, 3, oh, ow] on the device (out: the tensor to write).  Does not synchronise."""
        torch = self.torch
        self._bind_stream()
        sf, (n, H, W) = self._canvas_of(img)
        assert isinstance(lut, torch.Tensor) and lut.dtype == torch.float32 and lut.device == self.device and lut.is_contiguous() \
            and lut.numel() % 768 == 0 and tuple(lut.shape[-2:]) == (3, 256), "prep_images(lut=...): a contiguous float32 [nlut, 3, 256] tensor on the env's device"
        b = np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 3)
        li = None if lut_index is None else np.ascontiguousarray(lut_index, dtype=np.int32).reshape(len(b))
        si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32).reshape(len(b))
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if out is None:
            out = torch.empty((len(b), 3, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.device == self.device and tuple(out.shape) == (len(b), 3, oh, ow) and out.is_contiguous()
        check_call(self.h, self.L.avsim_image_prep(self.h.h, img.data_ptr(), sf, n, H, W, lut.data_ptr(), lut.numel() // 768, _ffi.ptr(li), b.ctypes.data,
                                                   len(b), _ffi.ptr(si), oh, ow, out.data_ptr()))
        return out

    def jitter_images(self, img, params, out_hw, mean=None, std=None, src_index=None, out=None):
        """Brightness, contrast, saturation, hue and sharpness jitter of img, cropped, mirrored and normalised in one pass (avsim_image_jitter;
        av_aloha_amd.imgaug.jitter_reference's bits).  img: a uint8 [n, H, W, 3] tensor on the env's device -- an observation, a decode_jpeg
        result --; params: HOST imgaug.PARAMS_DTYPE rows or the pair (int32 [nout, 4] = (x0, y0, flip, mask), float32 [nout, 5]); mean / std:
        three HOST values each, or None: the output stays in [0, 1]; src_index: a HOST int array, the source image of every output (None: image
        i).  All host arrays are checked (ValueError) and copied by the library before the call returns.  -> float32 [nout, 3, oh, ow] on the
        device (out: the tensor to write).  Does not synchronise."""
        from . import imgaug
        torch = self.torch
        self._bind_stream()
        assert isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.device == self.device and img.ndim == 4 and img.shape[3] == 3 \
            and img.is_contiguous(), "jitter_images(img=...): a contiguous uint8 [n, H, W, 3] tensor on the env's device"
        n, H, W = (int(v) for v in img.shape[:3])
        bm, fac = imgaug.split_params(params)
        si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32).reshape(len(bm))
        ms = imgaug.mean_std(mean, std)
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if out is None:
            out = torch.empty((len(bm), 3, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.device == self.device and tuple(out.shape) == (len(bm), 3, oh, ow) and out.is_contiguous()
        check_call(self.h, self.L.avsim_image_jitter(self.h.h, img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(si), len(bm), _ffi.ptr(ms), oh, ow,
                                                     out.data_ptr()))
        return out

    def augment_images(self, img, params, matrix, out_hw, interp=0, mean=None, std=None, src_index=None, out=None):
        """jitter_images with the geometric op, mask bit 5 (avsim_image_augment; av_aloha_amd.imgaug.jitter_affine_reference's bits).  matrix:
        HOST float32 [nout, 6], the inverse matrices (imgaug.affine_matrix) of the outputs that have the bit, or None when none has; interp: 0
        nearest, 1 bilinear.  Everything else as jitter_images.  Does not synchronise."""
        from . import imgaug
        torch = self.torch
        self._bind_stream()
        assert isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.device == self.device and img.ndim == 4 and img.shape[3] == 3 \
            and img.is_contiguous(), "augment_images(img=...): a contiguous uint8 [n, H, W, 3] tensor on the env's device"
        n, H, W = (int(v) for v in img.shape[:3])
        bm, fac = imgaug.split_params(params)
        mat = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float32).reshape(len(bm), 6)
        si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32).reshape(len(bm))
        ms = imgaug.mean_std(mean, std)
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if out is None:
            out = torch.empty((len(bm), 3, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.device == self.device and tuple(out.shape) == (len(bm), 3, oh, ow) and out.is_contiguous()
        check_call(self.h, self.L.avsim_image_augment(self.h.h, img.data_ptr(), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(mat), int(interp), _ffi.ptr(si), len(bm),
                                                      _ffi.ptr(ms), oh, ow, out.data_ptr()))
        return out


    def resize_images(self, img, src_box, dst, out_hw, antialias=True, fill=None, mean=None, std=None, src_index=None, out=None):
        """Regions of img resized by the triangle filter of interpolate(mode="bilinear", antialias=...) into rectangles of a padded output,
        mirrored and normalised in one pass (avsim_image_resize; av_aloha_amd.imgresize.resize_reference's bits).  img: a tensor on the env's
        device, uint8 [n, H, W, 3] or float32 [n, 3, H, W] (read as floats: a jitter_images result resizes without a loss); src_box: HOST int
        rows (x0, y0, w, h, flip), the source regions; dst: HOST int rows (ox, oy, rw, rh), where the resized regions go in the oh x ow
        output (imgresize.resize_with_pad_plan makes a letterbox); fill: three HOST values for every other pixel (None: 0); mean / std: three
        HOST values each, or None; src_index: a HOST int array, the source image of every output (None: image i).  All host arrays are
        checked (ValueError) and copied by the library before the call returns.  -> float32 [nout, 3, oh, ow] on the device (out: the tensor
        to write).  Does not synchronise."""
        from . import imgresize
        torch = self.torch
        self._bind_stream()
        sf, (n, H, W) = self._canvas_of(img)
        b = np.ascontiguousarray(src_box, dtype=np.int32).reshape(-1, 5)
        d = np.ascontiguousarray(dst, dtype=np.int32).reshape(len(b), 4)
        si = None if src_index is None else np.ascontiguousarray(src_index, dtype=np.int32).reshape(len(b))
        fl = None if fill is None else np.ascontiguousarray(fill, dtype=np.float32).reshape(3)
        ms = imgresize.mean_std(mean, std)
        oh, ow = int(out_hw[0]), int(out_hw[1])
        if out is None:
            out = torch.empty((len(b), 3, max(oh, 0), max(ow, 0)), dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.device == self.device and tuple(out.shape) == (len(b), 3, oh, ow) and out.is_contiguous()
        check_call(self.h, self.L.avsim_image_resize(self.h.h, img.data_ptr(), sf, n, H, W, b.ctypes.data, d.ctypes.data, _ffi.ptr(si), len(b), int(antialias),
                                                     _ffi.ptr(fl), _ffi.ptr(ms), oh, ow, out.data_ptr()))
        return out

class DeviceImages(DeviceImageOps):
    """DeviceImageOps for a caller that has no env: images go in and come out as tensors on `device`, and nothing is simulated.  The library
    has no handle without a model (that would take a new entry point, which is out of scope here), so this makes the smallest one it offers --
    one env of the InsertPeg model, of which the image calls use nothing -- and is the one place that does.  torch's GPU is touched first
    (vec_env.py says why).  decode_jpeg's fmt defaults to "lerobot"; its height and width have no default here."""

    obs_format, observation_height, observation_width = "lerobot", None, None

    def __init__(self, device=None):
        import torch
        from .sim import load_blob
        self.torch, self._stream = torch, None
        d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device if device is not None else "cuda")
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        torch.zeros(1, device=self.device)
        with torch.cuda.device(self.device):
            self.h = _ffi.Handle(load_blob("insert_peg", 3)[0], 1, self.device.index, _ffi.AVSIM_IO_DEVICE)
        self.L = self.h.L
