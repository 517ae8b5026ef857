"""What a policy with n_obs_steps = K > 1 reads: per-env histories [N, K, ...] of the prepared observations, restarted per env when its episode
is.

The numpy half of this module -- check_setup, ObsHistoryReference -- is the SPECIFICATION: host only, float32 throughout, every operation
rounded on its own.  The device (avsim_obs_history_*, csrc/avsim_obshist.hip) equals it bit for bit.  ObsHistory is the device call on torch
tensors for the owner of a device-I/O handle (vec_env.VecEnv); sim.BatchedSim.obs_history_setup / push / reset are the same on numpy arrays.

LeRobot keeps one observation queue for the whole batch: policy.reset() empties it and the next observation fills it with copies of itself
(populate_queues).  On the vector env an env that starts a new episode in the middle of the batch would get the last frame of its previous
episode stacked under its reset frame.  Here the state is per env.

Fresh: env i is fresh in a call when it has not been pushed since set-up or reset(), or elapsed[i] == 0, or episode_id[i] differs from the id
it had in the previous call -- chunks.ChunkReference's rule, for its reasons.

Per env and call: new_s = (state - mean) / std, two operations (without statistics: state); new_i[c] = imgprep.prep_reference(img, lut[c],
box[c]) -- one table and one (x0, y0, flip) per camera, fixed by the set-up; the sources are avsim_image_prep's two formats, u8 HWC and
float32 CHW through imgprep.to_u8.  A fresh env: all K slots become the new value, the old contents are not read (they may be NaN).
Otherwise slot[k] = slot[k+1] for k < K-1 and slot[K-1] = new: slot K-1 is the newest.  K = 1 is prep_reference itself."""
from __future__ import annotations

import numpy as np

from . import imgprep

MAX_STEPS, MAX_STATE_DIM, MAX_CAMERAS = 16, 256, 8
FORMATS = {"gym": 0, "lerobot": 1}


def mean_std(mean, std, D):
    """None, or float32 [2, D] = (mean, std) for the library; both or neither."""
    if mean is None and std is None:
        return None
    if mean is None or std is None:
        raise ValueError("obshist: give both mean and std, or neither")
    ms = np.stack([np.asarray(mean, dtype=np.float32).reshape(-1), np.asarray(std, dtype=np.float32).reshape(-1)])
    if ms.shape != (2, int(D)):
        raise ValueError(f"obshist: mean / std have {ms.shape[1]} values, state_dim is {D}")
    return np.ascontiguousarray(ms)


def check_setup(K, D, ncam=0, fmt=0, src_hw=None, out_hw=None, lut=None, box=None, mean=None, std=None):
    """ValueError for what avsim_obs_history_setup refuses -> (mean_std float32 [2, D] or None, lut float32 [ncam, 3, 256] or None, box int32
    [ncam, 3] or None).  fmt: 0 / "gym" (u8 [N, H, W, 3]) or 1 / "lerobot" (float32 [N, 3, H, W]); src_hw = (H, W), out_hw = (h, w)."""
    K, D, ncam = int(K), int(D), int(ncam)
    if not 1 <= K <= MAX_STEPS:
        raise ValueError(f"obshist: n_obs_steps {K} outside 1..{MAX_STEPS}")
    if not 0 <= D <= MAX_STATE_DIM:
        raise ValueError(f"obshist: state_dim {D} outside 0..{MAX_STATE_DIM}")
    if not 0 <= ncam <= MAX_CAMERAS:
        raise ValueError(f"obshist: {ncam} cameras, outside 0..{MAX_CAMERAS}")
    if D == 0 and ncam == 0:
        raise ValueError("obshist: neither a state nor a camera")
    ms = mean_std(mean, std, D) if D > 0 else None
    if ms is not None:
        if not np.isfinite(ms).all():
            raise ValueError("obshist: a state mean or std that is not finite")
        if (ms[1] == 0).any():
            raise ValueError("obshist: a state std that is 0")
    if ncam == 0:
        return ms, None, None
    if fmt not in (0, 1) and fmt not in FORMATS:
        raise ValueError(f"obshist: image format {fmt!r} (0 / 'gym' or 1 / 'lerobot')")
    if src_hw is None or out_hw is None or lut is None or box is None:
        raise ValueError("obshist: cameras need src_hw, out_hw, their tables and their boxes")
    (H, W), (h, w) = (int(v) for v in src_hw), (int(v) for v in out_hw)
    if not all(1 <= v <= 65535 for v in (H, W, h, w)):
        raise ValueError("obshist: a size outside 1..65535")
    lut = np.ascontiguousarray(lut, dtype=np.float32)
    if lut.shape != (ncam, 3, 256):
        raise ValueError(f"obshist: tables of shape {lut.shape}, expected {(ncam, 3, 256)}")
    box = np.ascontiguousarray(box, dtype=np.int64)
    if box.shape != (ncam, 3):
        raise ValueError(f"obshist: boxes of shape {box.shape}, expected {(ncam, 3)}")
    for c, (x0, y0, flip) in enumerate(box):
        if flip not in (0, 1):
            raise ValueError(f"obshist: camera {c}: flip is 0 or 1")
        if x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
            raise ValueError(f"obshist: camera {c}: the crop does not lie inside the source")
    return ms, lut, box.astype(np.int32)


class ObsHistoryReference:
    """The specification as a state machine over N envs (the module's docstring).  cams: the number of cameras (or their names).
    push(state, images, episode_id, elapsed) -> (state_hist, img_hist): state float32 [N, D] (None with D = 0), images one batch per camera;
    state_hist float32 [N, K, D] and img_hist[c] float32 [N, K, 3, h, w] are the object's own arrays, updated in place (they start as NaN:
    nothing reads them before an env's first push).  reset(): all envs unpushed."""

    def __init__(self, N, K, D, cams=0, fmt=0, src_hw=None, out_hw=None, lut=None, box=None, mean=None, std=None):
        self.ncam = len(cams) if hasattr(cams, "__len__") else int(cams)
        ms, self.lut, self.box = check_setup(K, D, self.ncam, fmt, src_hw, out_hw, lut, box, mean, std)
        self.N, self.K, self.D = int(N), int(K), int(D)
        if self.N < 1:
            raise ValueError("obshist: N >= 1")
        self.fmt = FORMATS.get(fmt, fmt)
        self.mean, self.std = (ms[0].copy(), ms[1].copy()) if ms is not None else (None, None)
        self.src_hw = None if self.ncam == 0 else (int(src_hw[0]), int(src_hw[1]))
        self.out_hw = None if self.ncam == 0 else (int(out_hw[0]), int(out_hw[1]))
        self.pushed = np.zeros(self.N, dtype=bool)
        self.last_id = np.zeros(self.N, dtype=np.int64)
        self.state_hist = np.full((self.N, self.K, self.D), np.nan, dtype=np.float32)
        self.img_hist = [np.full((self.N, self.K, 3) + self.out_hw, np.nan, dtype=np.float32) for _ in range(self.ncam)]

    def reset(self):
        self.pushed[:] = False

    def fresh(self, episode_id, elapsed):
        """bool [N]: the envs the next push with these ids and elapsed steps starts anew (changes nothing)"""
        episode_id = np.asarray(episode_id, dtype=np.int64).reshape(self.N)
        elapsed = np.asarray(elapsed, dtype=np.int32).reshape(self.N)
        return ~self.pushed | (elapsed == 0) | (episode_id != self.last_id)

    def _put(self, hist, new, fresh):
        keep = ~fresh
        for k in range(self.K - 1):
            hist[keep, k] = hist[keep, k + 1]
        hist[keep, self.K - 1] = new[keep]
        hist[fresh] = new[fresh][:, None]

    def push(self, state, images, episode_id, elapsed):
        fresh = self.fresh(episode_id, elapsed)
        if self.D > 0:
            s = np.asarray(state, dtype=np.float32)
            if s.shape != (self.N, self.D):
                raise ValueError(f"obshist: state of shape {s.shape}, expected {(self.N, self.D)}")
            if self.mean is not None:
                s = (s - self.mean) / self.std                      # float32: a subtraction, then a division
            self._put(self.state_hist, s, fresh)
        images = [] if images is None else list(images)
        if len(images) != self.ncam:
            raise ValueError(f"obshist: {len(images)} image batches for {self.ncam} cameras")
        for c, img in enumerate(images):
            u = imgprep.to_u8(img)
            if u.shape != (self.N,) + self.src_hw + (3,) or (np.asarray(img).dtype == np.uint8) != (self.fmt == 0):
                raise ValueError(f"obshist: camera {c}: images of shape {np.asarray(img).shape} do not match the set-up")
            new = imgprep.prep_reference(u, self.lut[c], None, np.tile(self.box[c], (self.N, 1)), self.out_hw)
            self._put(self.img_hist[c], new, fresh)
        self.pushed[:] = True
        self.last_id = np.asarray(episode_id, dtype=np.int64).reshape(self.N).copy()
        return self.state_hist, self.img_hist


class ObsHistory:
    """Per-env observation histories on the device (avsim_obs_history_*): one state per handle, so one ObsHistory per env object at a time.
    env: anything that holds a device-I/O handle the way vec_env.VecEnv does (h, L, device, torch, num_envs, _bind_stream).  cameras: their
    names (default: the env's), state_dim (default: the env's joint count; 0: no state), fmt "lerobot" / "gym" and size = (H, W) of the images
    (defaults: the env's observation format and size).  crop = (h, w): the centred box (None: the whole image); the table of a camera is
    imgprep.normalise_lut(stats) -- identity_lut() without stats -- and the state is normalised with stats["observation.state"]:
    harness.make_preprocessor's numbers, so n_obs_steps = 1 equals it bit for bit.  boxes / luts: {camera: (x0, y0, flip)} / {camera: float32
    [3, 256]} for a caller whose numbers are others.  Every call runs on torch's current stream and none synchronises.  ValueError for what
    the library refuses."""

    def __init__(self, env, n_obs_steps, stats=None, crop=None, cameras=None, state_dim=None, fmt=None, size=None, boxes=None, luts=None):
        from .images import check_call
        self._check = check_call
        self.env, self.torch = env, env.torch
        torch, dev = self.torch, env.device
        self.N, self.K = int(env.num_envs), int(n_obs_steps)
        self.cameras = list(getattr(env, "cameras", []) if cameras is None else cameras)
        self.D = int(env.nj if state_dim is None else state_dim)
        fmt = getattr(env, "obs_format", "lerobot") if fmt is None else fmt
        if fmt not in (0, 1) and fmt not in FORMATS:
            raise ValueError(f"obshist: image format {fmt!r} (0 / 'gym' or 1 / 'lerobot')")
        self.fmt = FORMATS.get(fmt, fmt)
        H, W = (env.observation_height, env.observation_width) if size is None else (int(size[0]), int(size[1]))
        h, w = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
        self.src_hw, self.out_hw = (H, W), (h, w)
        ncam = len(self.cameras)
        lut = box = None
        if ncam:
            x0, y0 = imgprep.center_box((H, W), (h, w))
            box = np.array([(boxes or {}).get(c, (x0, y0, 0)) for c in self.cameras], dtype=np.int32).reshape(ncam, 3)
            tabs = []
            for c in self.cameras:
                if luts is not None and c in luts:
                    tabs.append(np.asarray(luts[c], dtype=np.float32).reshape(3, 256))
                elif stats is not None:
                    st = stats[f"observation.images.{c}"]
                    tabs.append(imgprep.normalise_lut(st["mean"], st["std"]))
                else:
                    tabs.append(imgprep.identity_lut())
            lut = np.ascontiguousarray(np.stack(tabs), dtype=np.float32)
        mean = std = None
        if stats is not None and self.D > 0:
            mean, std = stats["observation.state"]["mean"], stats["observation.state"]["std"]
        ms = mean_std(mean, std, self.D) if self.D > 0 else None
        self.setup_args = dict(cams=ncam, fmt=self.fmt, src_hw=self.src_hw, out_hw=self.out_hw, lut=lut, box=box,
                               mean=None if ms is None else ms[0], std=None if ms is None else ms[1])
        env._bind_stream()
        self._check(env.h, env.L.avsim_obs_history_setup(env.h.h, self.K, self.D, None if ms is None else ms.ctypes.data, ncam, self.fmt, H, W,
                                                         None if lut is None else lut.ctypes.data, None if box is None else box.ctypes.data, h, w))
        # the outputs: preallocated, updated in place by every push
        self.out = {}
        if self.D > 0:
            self.out["observation.state"] = torch.zeros((self.N, self.K, self.D), dtype=torch.float32, device=dev)
        for c in self.cameras:
            self.out[f"observation.images.{c}"] = torch.zeros((self.N, self.K, 3, h, w), dtype=torch.float32, device=dev)
        import ctypes
        self._img_ptrs = (ctypes.c_void_p * max(ncam, 1))()
        self._hist_ptrs = (ctypes.c_void_p * max(ncam, 1))(*[self.out[f"observation.images.{c}"].data_ptr() for c in self.cameras])
        self._src_shape = (self.N, H, W, 3) if self.fmt == 0 else (self.N, 3, H, W)
        self._src_dtype = torch.uint8 if self.fmt == 0 else torch.float32

    def reference(self):
        """An ObsHistoryReference with this object's set-up."""
        return ObsHistoryReference(self.N, self.K, self.D, **self.setup_args)

    def push(self, obs, info):
        """obs: either observation format of VecEnv -- "observation.state" float32 [N, D] or "agent_pos" (cast to float32, as
        harness.make_preprocessor does); "observation.images.<cam>" or "pixels"[<cam>]: contiguous tensors of the set-up's shape on the env's
        device, the env's own or not.  info: "episode_id" int64 [N], "elapsed_steps" int32 [N].  -> {"observation.state": float32 [N, K, D],
        "observation.images.<cam>": float32 [N, K, 3, h, w]}: the preallocated tensors, which the next call updates.  The inputs are read
        before later work on the stream.  Does not synchronise."""
        env, torch = self.env, self.torch
        env._bind_stream()
        dev = env.device
        eid, el = info["episode_id"], info["elapsed_steps"]
        assert isinstance(eid, torch.Tensor) and eid.dtype == torch.int64 and eid.device == dev and tuple(eid.shape) == (self.N,) and eid.is_contiguous(), \
            "info['episode_id']: a contiguous int64 [N] tensor on the env's device"
        assert isinstance(el, torch.Tensor) and el.dtype == torch.int32 and el.device == dev and tuple(el.shape) == (self.N,) and el.is_contiguous(), \
            "info['elapsed_steps']: a contiguous int32 [N] tensor on the env's device"
        state = None
        if self.D > 0:
            state = obs["observation.state"] if "observation.state" in obs else obs["agent_pos"].to(torch.float32)
            assert isinstance(state, torch.Tensor) and state.dtype == torch.float32 and state.device == dev and tuple(state.shape) == (self.N, self.D), \
                f"the state: a float32 [{self.N}, {self.D}] tensor on the env's device"
            state = state.contiguous()
        for i, c in enumerate(self.cameras):
            key = f"observation.images.{c}"
            img = obs[key] if key in obs else obs["pixels"][c]
            assert isinstance(img, torch.Tensor) and img.dtype == self._src_dtype and img.device == dev and tuple(img.shape) == self._src_shape \
                and img.is_contiguous(), f"camera {c!r}: a contiguous {self._src_dtype} tensor of shape {self._src_shape} on the env's device"
            self._img_ptrs[i] = img.data_ptr()
        sh = self.out.get("observation.state")
        self._check(env.h, env.L.avsim_obs_history_push(env.h.h, eid.data_ptr(), el.data_ptr(), None if state is None else state.data_ptr(),
                                                        None if sh is None else sh.data_ptr(), self._img_ptrs, self._hist_ptrs))
        return self.out

    def reset(self):
        """All envs unpushed: every env is fresh in the next call.  Does not synchronise."""
        self.env._bind_stream()
        self._check(self.env.h, self.env.L.avsim_obs_history_reset(self.env.h.h))
