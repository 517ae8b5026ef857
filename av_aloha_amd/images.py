"""The device image calls of libavsim (include/avsim.h) from Python.  ImageCalls implements compose and label, image statistics, prep, jitter,
augment, resize, camera poses, label images, point clouds, voxel grids and virtual views once each, against one of two array adaptors: HostArrays (numpy; BatchedSim) and DeviceArrays
(torch tensors on a device; DeviceImageOps, which VecEnv inherits).  The adaptors hold all that differs between the fronts:
  * numpy converts what it is given (np.ascontiguousarray of the pixels, values= to int64, lut= to float32 [-1, 3, 256]); torch takes
    contiguous tensors of the right type on the owner's device and fails an assert for anything else;
  * a wrong `out` or canvas, a jitter / augment img that is not u8 HWC, a depth or rgb of the wrong shape: ValueError in numpy, AssertionError in torch;
  * image_stats returns uint64 and refuses an index outside [0, n) in numpy, returns int64 and clamps the index tensor in torch;
  * torch binds its current stream before a call and never synchronises; the numpy front's handle (host I/O mode) is synchronous by itself.
DeviceImageOps adds the JPEG calls on buffers, and DeviceImages is DeviceImageOps for a caller that has no env (a data set, a video tool)."""
import math
import operator

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
    s = a.shape
    if len(s) == 4:
        dtype = _DTYPE_NAME.get(a.dtype) or _DTYPE_NAME.setdefault(a.dtype, str(a.dtype).rsplit(".", 1)[-1])      # (str() of a dtype per call is slow)
        if dtype == "uint8" and s[3] == 3:
            return 0, int(s[0]), int(s[1]), int(s[2])
        if dtype == "float32" and s[1] == 3:
            return 1, int(s[0]), int(s[2]), int(s[3])
    raise ValueError("compose: images are uint8 [n, H, W, 3] or float32 [n, 3, H, W]")


def default_stride(L, H, W, divisor):
    """Bytes reserved per JPEG stream of an H x W image when the caller says nothing: the raw frame's over `divisor` in whole 4 KB, never
    more than the worst case (avsim_jpeg_bound)."""
    return int(min(L.avsim_jpeg_bound(H, W), (H * W * 3 // divisor + 4095) // 4096 * 4096))


def camera_ids(manifest, cameras):
    """int32 ids of cameras given by name (the manifest's camera table) or by index."""
    names = manifest["camera_names"]
    return np.array([names.index(c) if isinstance(c, str) else int(c) for c in cameras], dtype=np.int32)


# The two array adaptors of ImageCalls: namespaces, never instantiated; `o` is the owner of the call.
#   begin(o)                        before every call
#   empty(o, shape, dtype)          a new array (dtype by name)
#   ok(o, a, dtype, shape)          a is this front's kind of array, contiguous, [of this type] [and shape] [and on o's device]
#   fail(text, device_text)         how a violation is reported
#   ptr(a)                          its address, for an array that ok() has passed (_ffi.ptr asks again what kind of array it has and whether
#                                   it is contiguous, 0.3 us per tensor on the per-step path; _ffi.ptr stays for what may be None)
#   pixels(o, a)                    an image batch that is read
#   given(o, a, dtype, shape, ...)  a small input that follows the I/O mode (values, lut, depth)
#   stats_index(o, index, n)        image_stats's index

class HostArrays:
    """ImageCalls on numpy arrays in host memory (BatchedSim: a handle in host I/O mode, which copies in and out and waits by itself).
    What the caller gives is converted; what it must have got right -- an `out`, a canvas -- is a ValueError when it is not."""
    stats_dtype, ptr = "uint64", operator.attrgetter("ctypes.data")

    def begin(o):
        pass

    def empty(o, shape, dtype):
        return np.empty(shape, dtype=dtype)

    def ok(o, a, dtype=None, shape=None):
        return isinstance(a, np.ndarray) and a.flags.c_contiguous and (dtype is None or a.dtype == dtype) and (shape is None or a.shape == shape)

    def fail(text, device_text=None):
        raise ValueError(text)

    def pixels(o, a):
        return np.ascontiguousarray(a)                     # (a view, another memory order)

    def given(o, a, dtype, shape, device_text):
        a = np.ascontiguousarray(a, dtype=dtype)           # (a list, another type)
        return a if shape is None else a.reshape(shape)

    def stats_index(o, index, n):
        idx = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"image_stats: index outside [0, {n})")
        return idx


class DeviceArrays:
    """ImageCalls on torch tensors of the owner's device (DeviceImageOps: a handle in device I/O mode on torch's current stream, never
    synchronised).  Nothing is converted: a tensor of another type, shape or device, or one that is not contiguous, fails an assert."""
    stats_dtype, ptr, begin = "int64", operator.methodcaller("data_ptr"), operator.methodcaller("_bind_stream")

    def empty(o, shape, dtype):
        return o.torch.empty(shape, dtype=getattr(o.torch, dtype), device=o.device)

    def ok(o, a, dtype=None, shape=None):
        return isinstance(a, o.torch.Tensor) and a.device == o.device and a.is_contiguous() and (dtype is None or a.dtype == getattr(o.torch, dtype)) \
            and (shape is None or a.shape == shape)

    def fail(text, device_text=None):
        raise AssertionError(device_text or text)

    def pixels(o, a):
        return a

    def given(o, a, dtype, shape, device_text):            # (a leading -1 of shape: any leading extents, or none)
        assert isinstance(a, o.torch.Tensor) and a.device == o.device and a.is_contiguous() and a.dtype == getattr(o.torch, dtype) \
            and (shape is None or (a.shape[1 - len(shape):] == shape[1:] if shape[0] == -1 else a.shape == shape)), device_text
        return a

    def stats_index(o, index, n):
        assert isinstance(index, o.torch.Tensor) and index.dtype == o.torch.int32 and index.device == o.device and index.ndim == 1, \
            "image_stats(index=...): an int32 index tensor on the env's device"
        return index.clamp(0, n - 1).contiguous()


def _host(a, dtype, *shape):
    """A HOST argument of either front as a contiguous array of the C type, None as None.  (Bind it to a name: the library reads it during the call.)"""
    return None if a is None else np.ascontiguousarray(a, dtype=dtype).reshape(shape)


class ImageCalls:
    """Compose and label, image statistics, prep, jitter, augment, resize, camera poses, point clouds, voxel grids and virtual views: each call once, for the owner of a
    handle self.h (_ffi.Handle) -- and, for the camera calls, of a self.manifest -- whose self._arrays says what kind of array the pixels live
    in: HostArrays (numpy) or DeviceArrays (torch tensors on self.device).  The two kinds differ in what the adaptor holds and in nothing
    else: how an array is made, whether an input is converted or has to be right already, whether a wrong one is a ValueError or a failed
    assert, and what happens before a call (the torch front binds torch's current stream and never waits for it; the numpy front's handle is
    synchronous).  Arguments called HOST below are numpy arrays, lists or tuples on both fronts; the library checks them before it launches
    anything and copies them before the call returns.  AVSIM_EINVAL is a ValueError with the library's message, any other failure an
    AvsimError (check_call)."""

    _cam_major = 0          # what the owner keeps option "render_cam_major" at between calls (voxel_grid's own colour render is env-major)

    def _canvas(self, a):
        """(fmt, n, H, W) of an image batch that is written in place, so has to be this front's kind of array already."""
        A = self._arrays
        if not (A.ok(self, a) and a.ndim == 4):
            A.fail("compose: the canvas is a C-contiguous u8 [n, H, W, 3] or float32 [n, 3, H, W] array", "a contiguous 4-D tensor on the env's device")
        return layout(a)

    def _image(self, a):
        """(a, fmt, n, H, W) of an image batch that is read: numpy converts it (a view, another memory order), torch takes it as it is."""
        A = self._arrays
        a = A.pixels(self, a)
        if not (A.ok(self, a) and a.ndim == 4):
            A.fail("compose: images are uint8 [n, H, W, 3] or float32 [n, 3, H, W]", "a contiguous 4-D tensor on the env's device")
        return (a,) + layout(a)

    def _out(self, call, out, shape, dtype="float32", text="float32 [nout, 3, oh, ow]"):
        """`out`, or a new array, of exactly this type and shape (no out and a negative size: refused like a wrong out)."""
        A = self._arrays
        if out is None and min(shape) >= 0:
            return A.empty(self, shape, dtype)
        if not A.ok(self, out, dtype, shape):
            A.fail(f"{call}: out is a C-contiguous {text} array")
        return out

    def compose(self, src, places, out=None, canvas_hw=None, nout=None, clear=None, fmt=None):
        """Images resampled into rectangles of a canvas (avsim_compose; av_aloha_amd.compose.compose_reference's pixels).  src: uint8
        [n, H, W, 3] or float32 [n, 3, H, W] in [0, 1], a numpy array or a tensor on the env's device (an observation, a decode_jpeg result);
        places: HOST int rows (out image, src image, x0, y0, w, h).  out: the canvas (either format), written in place and returned; None:
        one of canvas_hw = (CH, CW) and nout images is made in format fmt ("gym" u8 HWC, the default, or "lerobot" float32 CHW) and cleared.
        clear: 0xRRGGBB to fill the canvas with first.  ValueError for what the library refuses (a rectangle outside the canvas, overlaps, a
        shrink of more than 16)."""
        A = self._arrays
        A.begin(self)
        p = _host(places, np.int32, -1, 6)
        src, sf, n, H, W = self._image(src)
        if out is None:
            if canvas_hw is None:
                raise ValueError("compose: give a canvas (out=...) or its size (canvas_hw=...)")
            if fmt not in (None, "gym", "lerobot"):
                raise ValueError(f"fmt {fmt!r}: 'lerobot' or 'gym'")
            nout = int(p[:, 0].max()) + 1 if nout is None and len(p) else int(nout or 1)
            CH, CW = int(canvas_hw[0]), int(canvas_hw[1])
            out = A.empty(self, (nout, 3, CH, CW), "float32") if fmt == "lerobot" else A.empty(self, (nout, CH, CW, 3), "uint8")
            clear = 0 if clear is None else clear
        df, no, CH, CW = self._canvas(out)
        check_call(self.h, self.h.L.avsim_compose(self.h.h, A.ptr(src), sf, n, H, W, A.ptr(out), df, no, CH, CW, p.ctypes.data, len(p),
                                                  0 if clear is None else 1, int(clear or 0) & 0xFFFFFF))
        return out

    def compose_label(self, canvas, where, prefix="", values=None, rgb=0xFFFFFF):
        """prefix + the decimal digits of values[i] painted at where[i] = (out image, x, y, scale) in the colour rgb (avsim_compose_label;
        av_aloha_amd.compose.label_reference's pixels).  The canvas (compose's) is written in place and returned; where: HOST rows; values:
        one integer per label, read by the kernel -- numpy: anything that converts to int64 [len(where)]; torch: an int64 tensor of that
        shape on the env's device, info["episode_id"] for one --, or None: the prefix alone."""
        A = self._arrays
        A.begin(self)
        df, no, CH, CW = self._canvas(canvas)
        w = _host(where, np.int32, -1, 4)
        if values is not None:
            values = A.given(self, values, "int64", (len(w),), "compose_label(values=...): a contiguous int64 tensor on the env's device, one value per label")
        check_call(self.h, self.h.L.avsim_compose_label(self.h.h, A.ptr(canvas), df, no, CH, CW, w.ctypes.data, len(w), prefix.encode("ascii", "replace"),
                                                        _ffi.ptr(values), int(rgb) & 0xFFFFFF))
        return canvas

    def image_stats(self, img, index=None, out=None):
        """(sum, sum of squares, min, max) of the u8 values per image and channel (avsim_image_stats; av_aloha_amd.imgprep.stats_reference's
        integers) -> [m, 3, 4], uint64 in numpy and int64 in torch (the values are below 2^63).  img: uint8 [n, H, W, 3] or float32
        [n, 3, H, W]; index: the images to reduce, in this order (None: all) -- numpy: int values, ValueError for one outside [0, n); torch:
        an int32 tensor on the env's device, clamped to that range.  out: the array to write."""
        A = self._arrays
        A.begin(self)
        img, sf, n, H, W = self._image(img)
        if index is not None:
            index = A.stats_index(self, index, n)
        m = n if index is None else int(index.shape[0])
        out = self._out("image_stats", out, (m, 3, 4), A.stats_dtype, A.stats_dtype + " [m, 3, 4]")
        check_call(self.h, self.h.L.avsim_image_stats(self.h.h, A.ptr(img), sf, _ffi.ptr(index), m, H, W, A.ptr(out)))
        return out

    def prep_images(self, img, lut, box, out_hw, lut_index=None, src_index=None, out=None):
        """Crops of img, mirrored where box says so, every channel through a table (avsim_image_prep; av_aloha_amd.imgprep.prep_reference's
        bits) -> float32 [nout, 3, oh, ow] (out: the array to write).  img: uint8 [n, H, W, 3] or float32 [n, 3, H, W]; lut: float32
        [nlut, 3, 256] or [3, 256] -- numpy: anything that converts and reshapes to that; torch: such a tensor on the env's device --; box:
        HOST int rows (x0, y0, flip), one per output; lut_index / src_index: HOST int arrays, the table / the source image of every output
        (None: table 0 / image i).  ValueError for what the library refuses (a crop outside the source, an index out of range)."""
        A = self._arrays
        A.begin(self)
        img, sf, n, H, W = self._image(img)
        lut = A.given(self, lut, "float32", (-1, 3, 256), "prep_images(lut=...): a contiguous float32 [nlut, 3, 256] tensor on the env's device")
        b = _host(box, np.int32, -1, 3)
        li, si = _host(lut_index, np.int32, len(b)), _host(src_index, np.int32, len(b))
        oh, ow = int(out_hw[0]), int(out_hw[1])
        out = self._out("prep_images", out, (len(b), 3, oh, ow))
        check_call(self.h, self.h.L.avsim_image_prep(self.h.h, A.ptr(img), sf, n, H, W, A.ptr(lut), math.prod(lut.shape) // 768, _ffi.ptr(li), b.ctypes.data, len(b),
                                                     _ffi.ptr(si), oh, ow, A.ptr(out)))
        return out

    def _jitter_args(self, call, img, params, out_hw, mean, std, src_index, out):
        """What jitter_images and augment_images marshal alike: (img, n, H, W, box_mask, factor, src_index, mean_std, oh, ow, out)."""
        from . import imgaug
        A = self._arrays
        A.begin(self)
        img = A.pixels(self, img)
        s = img.shape if A.ok(self, img, "uint8") else ()
        if not (len(s) == 4 and s[3] == 3):
            A.fail(f"{call}: the images are a u8 [n, H, W, 3] array", f"{call}(img=...): a contiguous uint8 [n, H, W, 3] tensor on the env's device")
        bm, fac = imgaug.split_params(params)
        oh, ow = int(out_hw[0]), int(out_hw[1])
        return (img, int(s[0]), int(s[1]), int(s[2]), bm, fac, _host(src_index, np.int32, len(bm)), imgaug.mean_std(mean, std), oh, ow,
                self._out(call, out, (len(bm), 3, oh, ow)))

    def jitter_images(self, img, params, out_hw, mean=None, std=None, src_index=None, out=None):
        """Brightness, contrast, saturation, hue and sharpness jitter of img, cropped, mirrored and normalised in one pass (avsim_image_jitter;
        av_aloha_amd.imgaug.jitter_reference's bits) -> float32 [nout, 3, oh, ow] (out: the array to write).  img: uint8 [n, H, W, 3], a
        numpy array or a tensor on the env's device; params: HOST imgaug.PARAMS_DTYPE rows or the pair (int32 [nout, 4] = (x0, y0, flip,
        mask), float32 [nout, 5] = the factors); mean / std: three HOST values each, or None: the output stays in [0, 1]; src_index: a HOST
        int array, the source image of every output (None: image i).  ValueError for what the library refuses."""
        A = self._arrays
        img, n, H, W, bm, fac, si, ms, oh, ow, out = self._jitter_args("jitter_images", img, params, out_hw, mean, std, src_index, out)
        check_call(self.h, self.h.L.avsim_image_jitter(self.h.h, A.ptr(img), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(si), len(bm), _ffi.ptr(ms), oh, ow,
                                                       A.ptr(out)))
        return out

    def augment_images(self, img, params, matrix, out_hw, interp=0, mean=None, std=None, src_index=None, out=None):
        """jitter_images with the geometric op, mask bit 5 (avsim_image_augment; av_aloha_amd.imgaug.jitter_affine_reference's bits).  matrix:
        HOST float32 [nout, 6], the inverse matrices (imgaug.affine_matrix) of the outputs that have the bit, or None when none has; interp: 0
        nearest, 1 bilinear.  Everything else as jitter_images."""
        A = self._arrays
        img, n, H, W, bm, fac, si, ms, oh, ow, out = self._jitter_args("augment_images", img, params, out_hw, mean, std, src_index, out)
        mat = _host(matrix, np.float32, len(bm), 6)
        check_call(self.h, self.h.L.avsim_image_augment(self.h.h, A.ptr(img), n, H, W, bm.ctypes.data, fac.ctypes.data, _ffi.ptr(mat), int(interp), _ffi.ptr(si), len(bm),
                                                        _ffi.ptr(ms), oh, ow, A.ptr(out)))
        return out

    def resize_images(self, img, src_box, dst, out_hw, antialias=True, fill=None, mean=None, std=None, src_index=None, out=None):
        """Regions of img resized by the triangle filter of interpolate(mode="bilinear", antialias=...) into rectangles of a padded output,
        mirrored and normalised in one pass (avsim_image_resize; av_aloha_amd.imgresize.resize_reference's bits) -> float32 [nout, 3, oh, ow]
        (out: the array to write).  img: uint8 [n, H, W, 3] or float32 [n, 3, H, W] (read as floats: a jitter_images result resizes without
        a loss); src_box: HOST int rows (x0, y0, w, h, flip), the source regions; dst: HOST int rows (ox, oy, rw, rh), where the resized
        regions go in the oh x ow output (imgresize.resize_with_pad_plan makes a letterbox); fill: three HOST values for every other pixel
        (None: 0); mean / std: three HOST values each, or None; src_index: a HOST int array, the source image of every output (None: image
        i).  ValueError for what the library refuses."""
        from . import imgresize
        A = self._arrays
        A.begin(self)
        img, sf, n, H, W = self._image(img)
        b = _host(src_box, np.int32, -1, 5)
        d = _host(dst, np.int32, len(b), 4)
        si, fl, ms = _host(src_index, np.int32, len(b)), _host(fill, np.float32, 3), imgresize.mean_std(mean, std)
        oh, ow = int(out_hw[0]), int(out_hw[1])
        out = self._out("resize_images", out, (len(b), 3, oh, ow))
        check_call(self.h, self.h.L.avsim_image_resize(self.h.h, A.ptr(img), sf, n, H, W, b.ctypes.data, d.ctypes.data, _ffi.ptr(si), len(b), int(antialias), _ffi.ptr(fl),
                                                       _ffi.ptr(ms), oh, ow, A.ptr(out)))
        return out

    def camera_poses(self, cameras):
        """float32 [N, len(cameras), 16]: the world pose of the named cameras at the current state (avsim_camera_poses) -- position pc[3],
        rotation Rc[9] (row major, camera frame to world, the camera looks along its -z), tan(fovy / 2), three zeros."""
        A = self._arrays
        A.begin(self)
        ids = camera_ids(self.manifest, cameras)
        out = A.empty(self, (self.h.num_envs, len(ids), 16), "float32")
        check_call(self.h, self.h.L.avsim_camera_poses(self.h.h, ids.ctypes.data, len(ids), A.ptr(out)))
        return out

    def label_table(self, kind="class"):
        """(table uint8 [ngeom + 1], names) of the owner's model: segment.label_table, made once per kind."""
        from . import segment
        cache = self.__dict__.setdefault("_label_tables", {})
        if kind not in cache:
            if "model" not in cache:
                cache["model"] = segment.read_model(self.manifest)
            cache[kind] = segment.label_table(self.manifest, cache["model"], kind)
        return cache[kind]

    def render_labels(self, cameras, height, width, kind="class", drop=(), depth=True, out=None):
        """(labels uint8 [N, len(cameras), height, width], depth float32 of the same shape or None): what every pixel of the named
        cameras' depth image shows at the current state (avsim_render_labels; av_aloha_amd.segment has the tables and the specification).
        kind: "class" (segment.FIXED_CLASSES, then the task's bodies; label_table("class")[1] names them), "body", "geom", or a table --
        HOST uint8 [ngeom + 1], the label of every collision geom and, last, of nothing.  drop: HOST class names (of a named kind) or label
        values; a pixel with such a label gets the far plane (30 m) as its depth, so that point_cloud, voxel_grid and virtual_views given
        this depth leave it out; labels keeps the true label.  Where nothing is dropped, depth is render_depth's image bit for bit.
        depth=False: no depth image (drop is then refused).  out: the label array to write.  ValueError for what the library refuses."""
        from . import segment
        A = self._arrays
        A.begin(self)
        ids = camera_ids(self.manifest, cameras)
        N, height, width = self.h.num_envs, int(height), int(width)
        table, names = self.label_table(kind) if isinstance(kind, str) else (np.ascontiguousarray(kind), None)
        flags = segment.drop_flags(drop, names)
        segment.check_labels(len(self.manifest["camera_names"]), len(self.manifest["geom_names"]), ids, height, width, table, flags, depth=bool(depth))
        shape = (N, len(ids), height, width)
        out = self._out("render_labels", out, shape, "uint8", "uint8 [N, cameras, height, width]")
        dep = A.empty(self, shape, "float32") if depth else None
        check_call(self.h, self.h.L.avsim_render_labels(self.h.h, ids.ctypes.data, len(ids), height, width, table.ctypes.data, _ffi.ptr(flags), _ffi.ptr(dep), A.ptr(out)))
        return out, dep

    def point_cloud(self, cameras, height, width, bounds, npoints, max_depth=None, depth=None):
        """(xyz float32 [N, P, 3], index int32 [N, P], count int32 [N, 2]): one cloud per env in the world frame from the depth images of the
        named cameras, cropped to HOST bounds (xlo ylo zlo xhi yhi zhi) and thinned by farthest point sampling (avsim_point_cloud): the bits of
        av_aloha_amd.pointcloud.point_cloud_reference given camera_poses().  depth: float32 [N, len(cameras), height, width] of the CURRENT
        state (None: rendered first); max_depth: None = the far plane, so that pixels that see nothing drop out.  index is the flat pixel
        slot * H * W + r * W + c, count = (candidates, distinct points).  ValueError for what the library refuses."""
        from . import pointcloud
        A = self._arrays
        A.begin(self)
        ids = camera_ids(self.manifest, cameras)
        N, P, height, width = self.h.num_envs, int(npoints), int(height), int(width)
        shape = (N, len(ids), height, width)
        if depth is None:
            depth = A.empty(self, shape, "float32")
            self.h.check(self.h.L.avsim_render_depth(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth)))
        text = "point_cloud(depth=...): a contiguous float32 [N, cameras, height, width] tensor on the env's device"
        depth = A.given(self, depth, "float32", None, text)
        if tuple(depth.shape) != shape:
            A.fail(f"point_cloud: depth is float32 {shape}, not {tuple(depth.shape)}", text)
        b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1)
        if b.shape != (6,):
            raise ValueError("point_cloud: bounds are xlo ylo zlo xhi yhi zhi")
        xyz, index, count = A.empty(self, (N, max(P, 0), 3), "float32"), A.empty(self, (N, max(P, 0)), "int32"), A.empty(self, (N, 2), "int32")
        check_call(self.h, self.h.L.avsim_point_cloud(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth), b.ctypes.data,
                                                      float(pointcloud.FAR_PLANE if max_depth is None else max_depth), P, A.ptr(xyz), A.ptr(index), A.ptr(count)))
        return xyz, index, count

    def voxel_grid(self, cameras, height, width, bounds, grid, max_depth=None, depth=None, rgb=None, colour=False, out=None):
        """float32 [N, gx, gy, gz, 8]: one dense grid per env over HOST bounds (xlo ylo zlo xhi yhi zhi, lo < hi) in the world frame, from the
        depth images of the named cameras (avsim_voxel_grid): the bits of av_aloha_amd.voxel.voxel_grid_reference given camera_poses().  A
        cell's channels: 0..2 the mean position of its points, 3..5 their mean colour in [0, 1] (0 without colour), 6 their number, 7
        occupancy 1.0 / 0.0; an empty cell is zeros.  grid: an int or three ints.  depth: float32 [N, len(cameras), height, width] of the
        CURRENT state (None: rendered first); rgb: uint8 [N, len(cameras), height, width, 3], the same pixels in avsim_render_rgb's env-major
        layout (None and colour=True: rendered first; None and colour=False: no colour); max_depth: None = the far plane.  out: the array
        to write.  The colour rendered here is what avsim_render_rgb draws for this owner -- the visual scene where one is loaded (a VecEnv
        with `cameras`), the collision proxies otherwise -- and always env-major: "render_cam_major" is switched off for that render and
        put back to self._cam_major, the value the owner keeps it at between calls (VecEnv: 1 with `cameras`; BatchedSim sets the option
        in each of its own render methods, 0 here).  An rgb that is GIVEN has to be env-major.  ValueError for what the library refuses."""
        from . import pointcloud, voxel
        A = self._arrays
        A.begin(self)
        ids = camera_ids(self.manifest, cameras)
        N, height, width = self.h.num_envs, int(height), int(width)
        g = np.array(voxel.grid_dims(grid), dtype=np.int32)
        if g.min() < 1 or g.max() > voxel.MAX_DIM or int(g[0]) * int(g[1]) * int(g[2]) > voxel.MAX_CELLS:      # (before an output of that size is made)
            raise ValueError(f"voxel_grid: grid dims are 1..{voxel.MAX_DIM} with at most 2^21 cells, not {tuple(int(x) for x in g)}")
        shape = (N, len(ids), height, width)
        if depth is None:
            depth = A.empty(self, shape, "float32")
            self.h.check(self.h.L.avsim_render_depth(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth)))
        if rgb is None and colour:          # env-major whatever the owner keeps "render_cam_major" at: switched off for this render, then put back
            rgb = A.empty(self, shape + (3,), "uint8")
            self.h.check(self.h.L.avsim_set_option(self.h.h, b"render_cam_major", 0.0))
            try:
                self.h.check(self.h.L.avsim_render_rgb(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(rgb)))
            finally:
                if self._cam_major:
                    self.h.check(self.h.L.avsim_set_option(self.h.h, b"render_cam_major", 1.0))
        text = "voxel_grid(depth=...): a contiguous float32 [N, cameras, height, width] tensor on the env's device"
        depth = A.given(self, depth, "float32", None, text)
        if tuple(depth.shape) != shape:
            A.fail(f"voxel_grid: depth is float32 {shape}, not {tuple(depth.shape)}", text)
        if rgb is not None:
            text = "voxel_grid(rgb=...): a contiguous uint8 [N, cameras, height, width, 3] tensor on the env's device"
            rgb = A.given(self, rgb, "uint8", None, text)
            if tuple(rgb.shape) != shape + (3,):
                A.fail(f"voxel_grid: rgb is uint8 {shape + (3,)}, not {tuple(rgb.shape)}", text)
        b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1)
        if b.shape != (6,):
            raise ValueError("voxel_grid: bounds are xlo ylo zlo xhi yhi zhi")
        out = self._out("voxel_grid", out, (N, int(g[0]), int(g[1]), int(g[2]), 8), text="float32 [N, gx, gy, gz, 8]")
        check_call(self.h, self.h.L.avsim_voxel_grid(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth), _ffi.ptr(rgb), b.ctypes.data,
                                                     float(pointcloud.FAR_PLANE if max_depth is None else max_depth), g.ctypes.data, A.ptr(out)))
        return out

    def virtual_views(self, cameras, height, width, bounds, views, size, radius=1, max_depth=None, depth=None, rgb=None, colour=False, out=None, index=None):
        """(out float32 [N, V, VH, VW, 8], index int32 [N, V, VH, VW]): V orthographic virtual images per env of the box HOST bounds (xlo ylo
        zlo xhi yhi zhi, lo < hi) in the world frame, z-buffered from the depth images of the named cameras (avsim_virtual_views): the bits of
        av_aloha_amd.virtviews.virtual_views_reference given camera_poses().  views: names ("+x" "-x" "+y" "-y" "+z" "-z": the face the box is
        seen from) or codes 0..5, 1 to 6 of them; size: an int or (VH, VW), 1..1024; radius: a point covers (2 radius + 1)^2 pixels, 0..4.  A
        pixel's channels: 0..2 the colour in [0, 1] of the nearest point that covers it (0 without colour), 3 its distance from the view's
        face, 4..6 its world position, 7 1.0; a pixel nothing covers is zeros.  index is the winner's flat source pixel slot * H * W + r * W + c
        (-1: none).  depth: float32 [N, len(cameras), height, width] of the CURRENT state (None: rendered first); rgb: uint8 [N, len(cameras),
        height, width, 3], the same pixels in avsim_render_rgb's env-major layout (None and colour=True: rendered first, env-major whatever
        the owner keeps "render_cam_major" at, as voxel_grid does; None and colour=False: no colour); max_depth: None = the far plane.  out,
        index: the arrays to write.  ValueError for what the library refuses."""
        from . import pointcloud, virtviews
        A = self._arrays
        A.begin(self)
        ids = camera_ids(self.manifest, cameras)
        N, height, width = self.h.num_envs, int(height), int(width)
        v = np.array(virtviews.view_codes(views), dtype=np.int32)
        sz = np.array(virtviews.view_size(size), dtype=np.int32)
        if not 1 <= len(v) <= virtviews.MAX_VIEWS or sz.min() < 1 or sz.max() > virtviews.MAX_SIZE:      # (before outputs of that size are made)
            raise ValueError(f"virtual_views: 1..{virtviews.MAX_VIEWS} views of 1..{virtviews.MAX_SIZE} pixels a side, not {len(v)} of {tuple(int(x) for x in sz)}")
        shape = (N, len(ids), height, width)
        if depth is None:
            depth = A.empty(self, shape, "float32")
            self.h.check(self.h.L.avsim_render_depth(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth)))
        if rgb is None and colour:          # env-major whatever the owner keeps "render_cam_major" at: switched off for this render, then put back
            rgb = A.empty(self, shape + (3,), "uint8")
            self.h.check(self.h.L.avsim_set_option(self.h.h, b"render_cam_major", 0.0))
            try:
                self.h.check(self.h.L.avsim_render_rgb(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(rgb)))
            finally:
                if self._cam_major:
                    self.h.check(self.h.L.avsim_set_option(self.h.h, b"render_cam_major", 1.0))
        text = "virtual_views(depth=...): a contiguous float32 [N, cameras, height, width] tensor on the env's device"
        depth = A.given(self, depth, "float32", None, text)
        if tuple(depth.shape) != shape:
            A.fail(f"virtual_views: depth is float32 {shape}, not {tuple(depth.shape)}", text)
        if rgb is not None:
            text = "virtual_views(rgb=...): a contiguous uint8 [N, cameras, height, width, 3] tensor on the env's device"
            rgb = A.given(self, rgb, "uint8", None, text)
            if tuple(rgb.shape) != shape + (3,):
                A.fail(f"virtual_views: rgb is uint8 {shape + (3,)}, not {tuple(rgb.shape)}", text)
        b = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1)
        if b.shape != (6,):
            raise ValueError("virtual_views: bounds are xlo ylo zlo xhi yhi zhi")
        vshape = (N, len(v), int(sz[0]), int(sz[1]))
        out = self._out("virtual_views", out, vshape + (8,), text="float32 [N, V, VH, VW, 8]")
        if index is not None and not A.ok(self, index, "int32", vshape):
            A.fail("virtual_views: index is a C-contiguous int32 [N, V, VH, VW] array")
        index = A.empty(self, vshape, "int32") if index is None else index
        check_call(self.h, self.h.L.avsim_virtual_views(self.h.h, ids.ctypes.data, len(ids), height, width, A.ptr(depth), _ffi.ptr(rgb), b.ctypes.data,
                                                        float(pointcloud.FAR_PLANE if max_depth is None else max_depth), v.ctypes.data, len(v), sz.ctypes.data, int(radius),
                                                        A.ptr(out), A.ptr(index)))
        return out, index


class DeviceImageOps(ImageCalls):
    """The image calls on torch tensors, for the owner of a device-I/O handle: ImageCalls through DeviceArrays, and the JPEG calls, which
    speak buffers here and lists of bytes in BatchedSim.  The owner has self.h (_ffi.Handle), self.L, self.device, self.torch, self._stream =
    None, and -- decode_jpeg's defaults -- self.obs_format, self.observation_height and self.observation_width.  Every call runs on torch's
    current stream (re-bound when it changes) and none synchronises it; close() waits for it and gives the handle back."""

    _arrays = DeviceArrays

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

    def voxel_grid(self, *args, channels_first=False, **kw):
        """ImageCalls.voxel_grid; channels_first=True returns the [N, 8, gx, gy, gz] view of the same memory (out.permute(0, 4, 1, 2, 3):
        channels_last_3d strides, which Conv3d takes as it is) -- no copy is made."""
        out = ImageCalls.voxel_grid(self, *args, **kw)
        return out.permute(0, 4, 1, 2, 3) if channels_first else out

    def virtual_views(self, *args, channels_first=False, **kw):
        """ImageCalls.virtual_views; channels_first=True returns out as the [N, V, 8, VH, VW] view of the same memory (out.permute(0, 1, 4,
        2, 3); its flatten(0, 1) is a channels_last [N V, 8, VH, VW] batch, which Conv2d takes as it is) -- no copy is made."""
        out, index = ImageCalls.virtual_views(self, *args, **kw)
        return (out.permute(0, 1, 4, 2, 3) if channels_first else out), index

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
        fmt, n, H, W = self._canvas(images)
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


class DeviceImages(DeviceImageOps):
    """DeviceImageOps for a caller that has no env: images go in and come out as tensors on `device`, and nothing is simulated.  The library
    has no handle without a model (that would take a new entry point, which is out of scope here), so this makes the smallest one it offers --
    one env of the InsertPeg model, of which the image calls use nothing -- and is the one place that does.  (It has no manifest and nothing
    to look at: ImageCalls's camera_poses and point_cloud are for an env.)  torch's GPU is touched first
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
