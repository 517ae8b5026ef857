"""BatchedSim: numpy-facing wrapper of a libavsim handle (host-pointer I/O mode).

This is the batched engine under the gym-style environments in env.py; every method is a direct call
into the C-ABI (include/avsim.h).  There is no CPU fallback.

compose, compose_label, image_stats, prep_images, jitter_images, augment_images, resize_images, camera_poses,
render_labels, point_cloud, voxel_grid and virtual_views are images.ImageCalls's -- the one implementation that the torch front (images.DeviceImageOps, VecEnv)
runs too -- through images.HostArrays: numpy arrays in and out, inputs converted with np.ascontiguousarray, a wrong
`out` or canvas a ValueError, image_stats in uint64 with its index checked, and no stream to bind (the handle is in
host I/O mode and synchronous).  The JPEG methods here speak lists of bytes and stay this class's own."""
import ctypes as C
import json
import os

import numpy as np

from . import _ffi, images
from .constants import MODEL_DIR, SIM_PHYSICS_ENV_STEP_RATIO

TASK_KEYS = ("insert_peg", "slot_insertion", "sew_needle", "tube_transfer", "hook_package")


VARIANT_PREFIX = {"gym": "", "data_collection": "dc_"}


def load_blob(task, num_arms, variant="gym"):
    """variant "gym": compiled from gym_guided_vision/gym_guided_vision/assets (the gym envs); "data_collection": from
    data_collection_scripts/assets, which sim_env.py loads (data_collection_scripts/constants.py:5): default solref on the needle
    and the peg, ZED fovy 90 (compiler --variant)."""
    base = os.path.join(MODEL_DIR, f"{VARIANT_PREFIX[variant]}{task}_{num_arms}arms")
    with open(base + ".avm", "rb") as f:
        blob = f.read()
    with open(base + ".json") as f:
        manifest = json.load(f)
    return blob, manifest


class BatchedSim(images.ImageCalls):
    _arrays = images.HostArrays       # compose ... point_cloud: images.ImageCalls's, on numpy arrays

    def __init__(self, task, num_arms=3, num_envs=1, device=0, f64=False, options=None, variant="gym", blob=None):
        assert task in TASK_KEYS, task
        file_blob, self.manifest = load_blob(task, num_arms, variant)
        blob = file_blob if blob is None else blob        # (tests: the task's model with an edited constant, e.g. gravity)
        self.h = _ffi.Handle(blob, num_envs, device, _ffi.AVSIM_F64_PHYSICS if f64 else 0)
        self.N = num_envs
        self._jpeg_stride = {}         # render_jpeg: the bytes reserved per stream of a shape, grown when a stream did not fit (a recorder calls per step)
        for k in ("nq", "nv", "nu", "nj", "nobj", "max_reward", "maxcon", "maxefc"):
            setattr(self, k, getattr(self.h, k))
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        self.h.check(self.h.L.avsim_set_option(self.h.h, name.encode(), float(value)))
        if name in ("maxcon", "maxefc"):       # the capacities size the contact export
            d = np.zeros(_ffi.NDIMS, dtype=np.int32)
            self.h.check(self.h.L.avsim_dims(self.h.h, d.ctypes.data))
            self.maxcon, self.maxefc = int(d[8]), int(d[9])

    def reset(self, obj_qpos, mask=None):
        obj = np.ascontiguousarray(obj_qpos, dtype=np.float64).reshape(self.N, self.nobj * 7)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self.h.check(self.h.L.avsim_reset(self.h.h, _ffi.ptr(m), obj.ctypes.data))

    def step(self, action, nsub=SIM_PHYSICS_ENV_STEP_RATIO, want_reward=True):
        a = np.ascontiguousarray(action, dtype=np.float32).reshape(self.N, self.nj)
        ap = np.empty((self.N, self.nj))
        rw = np.empty(self.N, dtype=np.int32) if want_reward else None
        su = np.empty(self.N, dtype=np.uint8) if want_reward else None
        self.h.check(self.h.L.avsim_step(self.h.h, a.ctypes.data, nsub, ap.ctypes.data, _ffi.ptr(rw), _ffi.ptr(su)))
        return ap, rw, (su.astype(bool) if su is not None else None)

    def step_ctrl(self, nsub=SIM_PHYSICS_ENV_STEP_RATIO):
        """nsub substeps driven by the ctrl vector as it stands (set_state / an earlier step): dm_control's physics.step(nsub)."""
        ap = np.empty((self.N, self.nj))
        rw = np.empty(self.N, dtype=np.int32)
        su = np.empty(self.N, dtype=np.uint8)
        self.h.check(self.h.L.avsim_step_ctrl(self.h.h, nsub, ap.ctypes.data, rw.ctypes.data, su.ctypes.data))
        return ap, rw, su.astype(bool)

    def step_cartesian(self, action23, ik_mode=_ffi.IK_REFERENCE, nsub=SIM_PHYSICS_ENV_STEP_RATIO):
        a = np.ascontiguousarray(action23, dtype=np.float64).reshape(self.N, 23)
        ap = np.empty((self.N, 21))
        rw = np.empty(self.N, dtype=np.int32)
        su = np.empty(self.N, dtype=np.uint8)
        self.h.check(self.h.L.avsim_step_cartesian(self.h.h, a.ctypes.data, ik_mode, nsub, ap.ctypes.data, rw.ctypes.data, su.ctypes.data))
        return ap, rw, su.astype(bool)

    def get_state(self):
        qpos, qvel = np.empty((self.N, self.nq)), np.empty((self.N, self.nv))
        ctrl, warm = np.empty((self.N, self.nu)), np.empty((self.N, self.nv))
        self.h.check(self.h.L.avsim_get_state(self.h.h, qpos.ctypes.data, qvel.ctypes.data, ctrl.ctypes.data, warm.ctypes.data))
        return qpos, qvel, ctrl, warm

    def set_state(self, qpos=None, qvel=None, ctrl=None, warm=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (qpos, qvel, ctrl, warm)]
        self.h.check(self.h.L.avsim_set_state(self.h.h, *[_ffi.ptr(a) for a in arrs]))

    def get_latch(self):
        """Per-env reward latch int32 [N] (SewNeedle's _threaded_needle, env.py:602): state next to qpos / qvel / ctrl."""
        l = np.empty(self.N, dtype=np.int32)
        self.h.check(self.h.L.avsim_get_latch(self.h.h, l.ctypes.data))
        return l

    def set_latch(self, latch):
        l = np.ascontiguousarray(latch, dtype=np.int32).reshape(self.N)
        self.h.check(self.h.L.avsim_set_latch(self.h.h, l.ctypes.data))

    def get_reset_poses(self):
        """[N, nobj, 7] object poses a diverged env is put back to (those of the episode's reset)."""
        o = np.empty((self.N, self.nobj, 7))
        self.h.check(self.h.L.avsim_get_reset_poses(self.h.h, o.ctypes.data))
        return o

    def set_reset_poses(self, poses):
        o = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.N, self.nobj, 7)
        self.h.check(self.h.L.avsim_set_reset_poses(self.h.h, o.ctypes.data))

    def set_qpos(self, qpos):
        q = np.ascontiguousarray(qpos, dtype=np.float64).reshape(self.N, self.nq)
        self.h.check(self.h.L.avsim_set_qpos(self.h.h, q.ctypes.data))

    def contacts(self):
        ncon = np.empty(self.N, dtype=np.int32)
        pairs = np.empty((self.N, self.maxcon, 2), dtype=np.int32)
        dist = np.empty((self.N, self.maxcon))
        self.h.check(self.h.L.avsim_get_contacts(self.h.h, ncon.ctypes.data, pairs.ctypes.data, dist.ctypes.data))
        return ncon, pairs, dist

    def render_depth(self, cameras, height, width):
        """Depth images float32 [N, len(cameras), height, width] (metres along the optical axis) of the named cameras
        (names from the manifest's camera table, or indices) at the current state."""
        ids = images.camera_ids(self.manifest, cameras)
        out = np.empty((self.N, len(ids), height, width), dtype=np.float32)
        self.h.check(self.h.L.avsim_render_depth(self.h.h, ids.ctypes.data, len(ids), height, width, out.ctypes.data))
        return out

    def load_visual(self, path=None):
        """The visual scene of render_rgb: the decimated mesh library models/visual_meshes.avv (compiler/vismesh.py) against the
        instances in the model blob; from then on render_rgb rasterises the visual meshes (robot, frame, textured table, task
        objects) instead of the collision proxies."""
        path = path or os.path.join(MODEL_DIR, "visual_meshes.avv")
        with open(path, "rb") as f:
            lib = f.read()
        self.h.check(self.h.L.avsim_load_visual(self.h.h, lib, len(lib)))
        self._visual = True

    def visual_info(self):
        """{triangles, vertices, overflow flags of the last visual render, instances in the model}."""
        info = np.zeros(4, dtype=np.int32)
        self.h.check(self.h.L.avsim_visual_info(self.h.h, info.ctypes.data))
        return dict(zip(("triangles", "vertices", "overflow", "instances"), (int(x) for x in info)))

    def render_rgb(self, cameras, height, width, visual=True, cam_major=False, out=None):
        """Colour images uint8 [N, len(cameras), height, width, 3] of the named cameras at the current state (the layout
        of the reference's "pixels" observation, env.py:180-188).  visual: the scene's visual meshes (loaded on first use from
        models/visual_meshes.avv); False: the collision proxies in flat colours (the depth renderer's geometry)."""
        if visual and not getattr(self, "_visual", False):
            self.load_visual()
        self.set_option("render_proxies", 0 if visual else 1)
        self.set_option("render_cam_major", 1 if (cam_major and visual) else 0)      # [len(cameras), N, height, width, 3]: every camera's batch contiguous
        ids = images.camera_ids(self.manifest, cameras)
        shape = (len(ids), self.N, height, width, 3) if (cam_major and visual) else (self.N, len(ids), height, width, 3)
        if out is None:
            out = np.empty(shape, dtype=np.uint8)
        else:           # the caller's own memory (a slice of a data set's image array): no copy after the one from the device
            assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == int(np.prod(shape)), "render_rgb(out=...): a C-contiguous uint8 array of the result's size"
        self.h.check(self.h.L.avsim_render_rgb(self.h.h, ids.ctypes.data, len(ids), height, width, out.ctypes.data))
        if visual:
            ov = self.visual_info()["overflow"]
            if ov:          # the image lacks triangles: say so instead of handing a policy a silently incomplete observation
                import warnings
                warnings.warn(f"avsim_render_rgb: a view ran out of {'triangle records' if ov & 1 else ''}{' and ' if ov == 3 else ''}{'tile-list entries' if ov & 2 else ''} "
                              f"at {height}x{width}: triangles were dropped from the image", RuntimeWarning, stacklevel=2)
        return out

    def encode_jpeg(self, frames_u8, quality=90):
        """JPEG streams (a list of bytes) of u8 frames [n, H, W, 3] -- or one [H, W, 3] --, encoded on the device (avsim_jpeg_encode): the
        bytes of av_aloha_amd.jpeg.encode_reference.  The frames go to the device and only the streams come back."""
        f = np.ascontiguousarray(frames_u8)
        if f.ndim == 3:
            f = f[None]
        if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
            raise ValueError("encode_jpeg takes u8 frames [n, H, W, 3]")
        n, H, W, _ = f.shape
        L, out = self.h.L, []
        bound = int(L.avsim_jpeg_bound(H, W))
        if bound < 0:
            raise ValueError(f"encode_jpeg: frame size {H} x {W}")
        batch = max(1, min(n, (256 << 20) // (H * W * 3)))

        def run(frames, stride):
            buf = np.empty((len(frames), stride), dtype=np.uint8)
            ln = np.empty(len(frames), dtype=np.int32)
            self.h.check(L.avsim_jpeg_encode(self.h.h, frames.ctypes.data, 0, None, len(frames), H, W, int(quality), buf.ctypes.data, stride, ln.ctypes.data))
            return buf, ln
        for i0 in range(0, n, batch):
            frames = f[i0:i0 + batch]
            buf, ln = run(frames, images.default_stride(L, H, W, 4))
            if int(ln.max()) > buf.shape[1]:          # some stream did not fit: its length says what it needs
                buf, ln = run(frames, int(ln.max()))
            out += [buf[i, :ln[i]].tobytes() for i in range(len(frames))]
        return out

    def render_jpeg(self, cameras, height, width, quality=90, tile=False):
        """render_rgb's visual-scene images as JPEG streams (avsim_render_jpeg): rendered and encoded on the device, only the streams come to
        the host -- the bytes encode_jpeg gives for render_rgb's frames.  -> [N][len(cameras)] bytes; tile: the cameras' views of an env side
        by side in one height x (len(cameras) * width) image, -> [N] bytes."""
        if not getattr(self, "_visual", False):
            self.load_visual()
        self.set_option("render_proxies", 0)
        self.set_option("render_cam_major", 0)
        ids = images.camera_ids(self.manifest, cameras)
        L = self.h.L
        iw = width * len(ids) if tile else width
        bound = int(L.avsim_jpeg_bound(height, iw))
        if bound < 0:
            raise ValueError(f"render_jpeg: image size {height} x {iw}")
        n = self.N if tile else self.N * len(ids)
        key = (height, iw, int(quality))
        strides = self._jpeg_stride
        stride = strides.get(key) or images.default_stride(L, height, iw, 8)
        while True:
            buf, ln = np.empty((n, stride), dtype=np.uint8), np.empty(n, dtype=np.int32)
            self.h.check(L.avsim_render_jpeg(self.h.h, ids.ctypes.data, len(ids), height, width, 1 if tile else 0, int(quality), buf.ctypes.data, stride, ln.ctypes.data))
            if int(ln.max()) <= stride:
                break
            stride = strides[key] = min(bound, int(ln.max()) * 5 // 4)        # some stream did not fit: its length says what it needs
        if self.visual_info()["overflow"]:
            import warnings
            warnings.warn(f"avsim_render_jpeg: a view ran out of triangle records or tile-list entries at {height}x{width}: triangles were dropped from the image", RuntimeWarning, stacklevel=2)
        out = [buf[i, :ln[i]].tobytes() for i in range(n)]
        return out if tile else [out[e * len(ids):(e + 1) * len(ids)] for e in range(self.N)]

    def decode_jpeg(self, streams, upsample="replicate"):
        """u8 frames [n, H, W, 3] of JPEG streams (a list of bytes, all of one size) that encode_jpeg / av_aloha_amd.jpeg.encode_reference
        wrote, decoded on the device (avsim_jpeg_decode): the pixels of av_aloha_amd.jpeg.decode_reference.  Raises ValueError (a
        jpeg.JpegError carrying the status) for a stream the decoder flags: it reads this encoder's streams and no others."""
        from . import jpeg
        if upsample not in ("replicate", "triangle"):
            raise ValueError(f"upsample {upsample!r}: 'replicate' or 'triangle'")
        streams = [bytes(s) for s in streams]
        if not streams:
            raise ValueError("decode_jpeg: no streams")
        H, W = jpeg.stream_size(streams[0])
        L = self.h.L
        out = np.empty((len(streams), H, W, 3), dtype=np.uint8)
        batch = max(1, (256 << 20) // (H * W * 3))
        for i0 in range(0, len(streams), batch):
            part = streams[i0:i0 + batch]
            stride = max(len(s) for s in part)
            buf, ln = np.zeros((len(part), stride), dtype=np.uint8), np.array([len(s) for s in part], dtype=np.int32)
            for i, s in enumerate(part):
                buf[i, :len(s)] = np.frombuffer(s, np.uint8)
            status = np.zeros(len(part), dtype=np.int32)
            self.h.check(L.avsim_jpeg_decode(self.h.h, buf.ctypes.data, stride, ln.ctypes.data, None, len(part), H, W, 0,
                                             1 if upsample == "triangle" else 0, out[i0:i0 + batch].ctypes.data, status.ctypes.data))
            if status.any():
                i = int(np.nonzero(status)[0][0])
                raise jpeg.JpegError(int(status[i]), f"decode_jpeg: stream {i0 + i} is not a {H} x {W} stream of this encoder (status {int(status[i])}: "
                                                     "1 header, 2 marker structure or length, 4 entropy-coded data)")
        return out

    def jitter_gray_sums(self, nout):
        """uint64 [nout]: the integer sums behind the contrast means of the last jitter_images call (avsim_image_jitter_sums;
        imgaug.gray_sum_reference's), meaningful for the outputs that had the contrast bit.  For tests."""
        sums = np.zeros(int(nout), dtype=np.uint64)
        images.check_call(self.h, self.h.L.avsim_image_jitter_sums(self.h.h, sums.ctypes.data, int(nout)))
        return sums

    def chunk_setup(self, chunk_size, action_dim=None, ensemble=None, n_action_steps=None, first=0, mean=None, std=None):
        """Per-env execution of action chunks on host arrays (avsim_chunk_setup; av_aloha_amd.chunks is the specification and
        chunks.ActionChunks the torch front): ensemble None -> a queue of n_action_steps (default chunk_size) rows from row `first`, a
        coefficient -> temporal ensembling with chunks.ensemble_tables; mean / std un-normalise the chunks.  ValueError for what the library
        refuses.  -> the keyword arguments of a chunks.ChunkReference(N, C, A, ...) of the same set-up."""
        from . import chunks
        C, A = int(chunk_size), int(self.nj if action_dim is None else action_dim)
        if ensemble is None:
            mode, tables, n_action_steps = "queue", None, (C if n_action_steps is None else n_action_steps)
        else:
            mode, tables = "ensemble", (chunks.ensemble_tables(C, ensemble) if 1 <= C <= chunks.MAX_CHUNK else None)
        ms = chunks.mean_std(mean, std, A)
        images.check_call(self.h, self.h.L.avsim_chunk_setup(self.h.h, C, A, chunks.MODES[mode], int(n_action_steps or 0), int(first), _ffi.ptr(tables), _ffi.ptr(ms)))
        self._chunk_shape = (C, A)
        return dict(mode=mode, tables=tables, n_action_steps=n_action_steps, first=first, mean=None if ms is None else ms[0], std=None if ms is None else ms[1])

    def _chunk_ids(self, episode_id, elapsed):
        eid = np.ascontiguousarray(episode_id, dtype=np.int64).reshape(self.N)
        return eid, np.ascontiguousarray(elapsed, dtype=np.int32).reshape(self.N)

    def chunk_need(self, episode_id, elapsed):
        """(need bool [N], any bool): the envs that need a chunk in the next chunk_step given these ids and elapsed steps (avsim_chunk_need)."""
        eid, el = self._chunk_ids(episode_id, elapsed)
        need, flag = np.zeros(self.N, dtype=np.uint8), np.zeros(1, dtype=np.int32)
        images.check_call(self.h, self.h.L.avsim_chunk_need(self.h.h, eid.ctypes.data, el.ctypes.data, need.ctypes.data, flag.ctypes.data))
        return need.astype(bool), bool(flag[0])

    def chunk_step(self, chunks, episode_id, elapsed):
        """float32 [N, A]: the actions of this call (avsim_chunk_step).  chunks: float32 [N, C, A], or None in queue mode."""
        if not hasattr(self, "_chunk_shape"):
            raise ValueError("chunk_step: call chunk_setup first")
        C, A = self._chunk_shape
        eid, el = self._chunk_ids(episode_id, elapsed)
        if chunks is not None:
            chunks = np.ascontiguousarray(chunks, dtype=np.float32)
            if chunks.shape != (self.N, C, A):
                raise ValueError(f"chunk_step: chunks of shape {chunks.shape}, expected {(self.N, C, A)}")
        action = np.zeros((self.N, A), dtype=np.float32)
        images.check_call(self.h, self.h.L.avsim_chunk_step(self.h.h, _ffi.ptr(chunks), eid.ctypes.data, el.ctypes.data, action.ctypes.data))
        return action

    def chunk_reset(self):
        images.check_call(self.h, self.h.L.avsim_chunk_reset(self.h.h))

    def chunk_starved(self):
        c = np.zeros(1, dtype=np.uint64)
        images.check_call(self.h, self.h.L.avsim_chunk_starved(self.h.h, c.ctypes.data))
        return int(c[0])

    def obs_history_setup(self, n_obs_steps, state_dim=None, mean=None, std=None, fmt=0, src_hw=None, out_hw=None, lut=None, box=None):
        """Per-env observation histories on host arrays (avsim_obs_history_setup; av_aloha_amd.obshist is the specification and
        obshist.ObsHistory the torch front).  state_dim defaults to the joint count (0: no state); mean / std normalise the state; lut float32
        [ncam, 3, 256] and box int (x0, y0, flip) rows: one table and one crop of out_hw = (h, w) per camera of src_hw = (H, W) images in
        format fmt (0: u8 HWC, 1: float32 CHW); lut None: no cameras.  ValueError for what the library refuses.  -> the keyword arguments of an
        obshist.ObsHistoryReference(N, K, D, ...) of the same set-up.  The histories live in this object (NaN until an env's first push)."""
        from . import obshist
        K, D = int(n_obs_steps), int(self.nj if state_dim is None else state_dim)
        ms = obshist.mean_std(mean, std, D) if D > 0 else None
        lut = None if lut is None else np.ascontiguousarray(lut, dtype=np.float32).reshape(-1, 3, 256)
        ncam = 0 if lut is None else len(lut)
        box = None if box is None else np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 3)
        if ncam and (box is None or len(box) != ncam or src_hw is None or out_hw is None):
            raise ValueError("obs_history_setup: cameras need src_hw, out_hw and one box per table")
        fmt = obshist.FORMATS.get(fmt, fmt)
        (H, W), (h, w) = (src_hw, out_hw) if ncam else ((0, 0), (0, 0))
        images.check_call(self.h, self.h.L.avsim_obs_history_setup(self.h.h, K, D, _ffi.ptr(ms), ncam, int(fmt) if ncam else 0, int(H), int(W), _ffi.ptr(lut), _ffi.ptr(box),
                                                                   int(h), int(w)))
        self._obs_hist = (np.full((self.N, K, D), np.nan, dtype=np.float32), [np.full((self.N, K, 3, int(h), int(w)), np.nan, dtype=np.float32) for _ in range(ncam)])
        self._obs_src = ((self.N, int(H), int(W), 3), np.uint8) if fmt == 0 else ((self.N, 3, int(H), int(W)), np.float32)
        return dict(cams=ncam, fmt=fmt, src_hw=src_hw, out_hw=out_hw, lut=lut, box=box, mean=None if ms is None else ms[0], std=None if ms is None else ms[1])

    def obs_history_push(self, state, imgs, episode_id, elapsed):
        """(state_hist float32 [N, K, D], [img_hist float32 [N, K, 3, h, w] per camera]) after this call's observations (avsim_obs_history_push):
        this object's arrays, updated in place.  state: float32 [N, D] (None with state_dim 0); imgs: one batch per camera."""
        import ctypes
        if not hasattr(self, "_obs_hist"):
            raise ValueError("obs_history_push: call obs_history_setup first")
        sh, ih = self._obs_hist
        eid, el = self._chunk_ids(episode_id, elapsed)
        D = sh.shape[2]
        if D > 0:
            state = np.ascontiguousarray(state, dtype=np.float32)
            if state.shape != (self.N, D):
                raise ValueError(f"obs_history_push: state of shape {state.shape}, expected {(self.N, D)}")
        imgs = [] if imgs is None else [np.ascontiguousarray(a) for a in imgs]
        shape, dtype = self._obs_src
        if len(imgs) != len(ih) or any(a.shape != shape or a.dtype != dtype for a in imgs):
            raise ValueError(f"obs_history_push: {len(ih)} image batches of shape {shape} and type {np.dtype(dtype).name}")
        src = (ctypes.c_void_p * max(len(ih), 1))(*[a.ctypes.data for a in imgs])
        dst = (ctypes.c_void_p * max(len(ih), 1))(*[a.ctypes.data for a in ih])
        images.check_call(self.h, self.h.L.avsim_obs_history_push(self.h.h, eid.ctypes.data, el.ctypes.data, state.ctypes.data if D > 0 else None,
                                                                  sh.ctypes.data if D > 0 else None, src, dst))
        return sh, ih

    def obs_history_reset(self):
        images.check_call(self.h, self.h.L.avsim_obs_history_reset(self.h.h))

    def reward_from_pairs(self, geom_pairs, latch=None):
        """The task's get_reward (env.py:425-863) on explicit contact lists: geom_pairs int [nsets, cap, 2] (collision
        geom ids, negative = empty slot); latch int32 [nsets] is updated in place.  Returns int32 [nsets]."""
        p = np.ascontiguousarray(geom_pairs, dtype=np.int32)
        assert p.ndim == 3 and p.shape[2] == 2
        if latch is not None:
            assert latch.dtype == np.int32 and latch.shape == (p.shape[0],) and latch.flags.c_contiguous
        rw = np.empty(p.shape[0], dtype=np.int32)
        self.h.check(self.h.L.avsim_reward_from_pairs(self.h.h, p.ctypes.data, p.shape[0], p.shape[1],
                                                      latch.ctypes.data if latch is not None else None, rw.ctypes.data))
        return rw

    def diag(self):
        d = np.empty((self.N, 4), dtype=np.int32)
        self.h.check(self.h.L.avsim_get_diag(self.h.h, d.ctypes.data))
        return d

    def close(self):
        self.h.close()
