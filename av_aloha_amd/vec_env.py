"""Device-resident vector env: the batch of env.py's facade with every observation, reward and flag kept in torch tensors on the GPU,
per-env episodes and gymnasium's NEXT_STEP autoreset done by the library's kernels (avsim_episode_*, include/avsim.h).

    env = make_vec("gym_guided_vision/InsertPeg-3Arms-v0", num_envs=256, max_episode_steps=300)
    obs, info = env.reset(seed=0)
    obs, reward, terminated, truncated, info = env.step(action)      # action: float32 [N, nj] on env.device

* obs_format "lerobot" (eval.py:23-66 preprocess_observation, done by the rasteriser): `observation.images.<cam>` float32 [N, 3, H, W] in
  [0, 1] (a contiguous view of the camera-major image batch) and `observation.state` float32 [N, nj]; "gym": GuidedVisionEnv's keys,
  `pixels[cam]` uint8 [N, H, W, 3] and `agent_pos` float64 [N, nj].  depth_cameras adds `depth[cam]` float32 [N, H, W].
* pointcloud={"cameras": [...], "height": h, "width": w, "bounds": (xlo, ylo, zlo, xhi, yhi, zhi), "points": P, "max_depth": None} adds
  `observation.pointcloud` (gym format: `pointcloud`) float32 [N, P, 3]: the cameras' depth rendered at its own size into its own buffer,
  deprojected into the world frame, cropped and thinned by farthest point sampling (avsim_point_cloud); `info["pointcloud_count"]` int32
  [N, 2] = (candidates, distinct points) and `info["pointcloud_index"]` int32 [N, P], the flat pixels.  None (the default): no call, buffer
  or key changes.
* voxels={"cameras": [...], "height": h, "width": w, "bounds": (xlo, ylo, zlo, xhi, yhi, zhi), "grid": g or (gx, gy, gz), "colour": False,
  "max_depth": None} adds `observation.voxels` (gym format: `voxels`) float32 [N, 8, gx, gy, gz], a channels_last_3d view of the
  [N, gx, gy, gz, 8] buffer that avsim_voxel_grid writes: per cell the mean position, the mean colour, the count and the occupancy.  The
  depth, and with "colour" the u8 colour images, are rendered at the option's own size into its own buffers.  Refused together with the
  "render_cam_major" option -- which `cameras` switch on --: the grid reads env-major images.  None (the default): no call, buffer or key changes.
* views={"cameras": [...], "height": h, "width": w, "bounds": (xlo, ylo, zlo, xhi, yhi, zhi), "views": ["+z", "+x", "-x", "+y", "-y"], "size": 220 or
  (vh, vw), "radius": 1, "colour": True, "max_depth": None} adds `observation.virtual_views` (gym format: `virtual_views`) float32
  [N, V, 8, VH, VW], a view of the [N, V, VH, VW, 8] buffer that avsim_virtual_views writes: RVT's orthographic images of the box, per pixel
  the nearest point's colour, its distance from the view's face, its world position and a hit flag; `info["virtual_views_index"]` int32
  [N, V, VH, VW] is the winning source pixel (-1: none).  The depth, and with "colour" the u8 colour images, are rendered at the option's own
  size into its own buffers.  Refused together with "render_cam_major" / `cameras`, as voxels are; allowed next to pointcloud and voxels.
  None (the default): no call, buffer or key changes.
* segmentation={"cameras": [...], "height": h, "width": w, "kind": "class"} adds `observation.segmentation` uint8 [N, ncam, h, w] (gym
  format: `segmentation[cam]` uint8 [N, h, w]): what every pixel of those cameras' depth image shows (avsim_render_labels into its own
  buffer; av_aloha_amd/segment.py has the tables), and `env.segmentation_classes`, the names of the labels.  pointcloud, voxels and views
  accept "drop": [class names] -- their depth buffer is then filled by avsim_render_labels with those classes at the far plane, so the
  robot (segment.ROBOT_CLASSES) leaves the cloud, the grid or the views --, and pointcloud also "labels": True, which adds
  `info["pointcloud_label"]` uint8 [N, P]: the class of every point (255 where `pointcloud_index` is -1).  None / no "drop" (the defaults): no
  call, buffer or key changes.
* Every tensor returned is a preallocated buffer that the next reset / step overwrites: clone what must outlive the call.
* NEXT_STEP: an env whose episode ended (terminated or truncated) in call t starts its next episode in call t + 1, whose action does
  not reach it; that call reports reward 0, flags 0, elapsed 0, the new `info["episode_id"]` and the new episode's first observation.
  A change of an env's episode id is the signal for per-env policy state (chunks.ActionChunks / harness.chunked_policy keep a chunked
  policy's queue or temporal ensembler per env on the device and restart it on that signal).
* Initial object poses come from Philox4x32-10 keyed by (seed, episode id) inside the library (OBJECT_BOXES below), not from the global
  numpy RNG that env.py's sample_object_poses consumes like the reference: an episode's poses do not depend on the batch size.
* torch's GPU must be initialised in the process before the first libavsim handle is created (torch ships its own HIP runtime
  next to the one libavsim links; the one that comes up second finds no device): import torch and touch the GPU first.
* No call synchronises the stream it runs on (torch's current stream, re-bound when it changes); check_render_overflow() reads the
  rasteriser's overflow flags once, where a per-step check would synchronise.
"""
from __future__ import annotations

import os
import warnings

import numpy as np

from . import _ffi
from .constants import CAMERAS, MODEL_DIR, SIM_PHYSICS_ENV_STEP_RATIO
from .env import ENVS
from .images import DeviceImageOps, camera_ids, default_stride
from .sim import load_blob

# Initial positions of the free objects in qpos order: (lo xyz, hi xyz) of the reference's uniform draws (env.py:474-501, 513-543,
# 604-637, 705-735, 792-818; the same ranges as env.sample_object_poses), and the earlier object whose draw an object shares.
OBJECT_BOXES = {
    "insert_peg": ([[0.1, -0.1, 0.01, 0.2, 0.1, 0.01], [-0.1, -0.1, 0.021, -0.2, 0.1, 0.021]], [-1, -1]),
    "slot_insertion": ([[-0.05, 0.1, 0.0, 0.05, 0.15, 0.0], [-0.08, -0.1, 0.0, 0.08, 0.0, 0.0]], [-1, -1]),
    "sew_needle": ([[-0.025, -0.025, 0.0, 0.025, 0.1, 0.0], [0.15, -0.025, 0.0, 0.2, 0.1, 0.0]], [-1, -1]),
    "tube_transfer": ([[0.05, -0.05, 0.0, 0.1, 0.05, 0.0], [0.05, -0.05, 0.0, 0.1, 0.05, 0.0], [-0.1, -0.05, 0.0, -0.05, 0.05, 0.0]],
                      [-1, 0, -1]),     # ball and tube1 share one draw
    "hook_package": ([[-0.1, 0.3, 0.2, 0.1, 0.3, 0.3], [-0.1, 0.0, 0.0, 0.1, 0.15, 0.0]], [-1, -1]),
}

_TASK_OF_CLASS = {"InsertPegEnv": "insert_peg", "SlotInsertionEnv": "slot_insertion", "SewNeedleEnv": "sew_needle",
                  "TubeTransferEnv": "tube_transfer", "HookPackageEnv": "hook_package"}


def philox4x32_10(ctr, key):
    """Random123's philox4x32-10 on uint32 arrays: ctr [..., 4], key [..., 2] -> [..., 4] (the library's avs::philox4x32_10)."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., j] for j in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[..., j] for j in range(2))
    m32 = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
    return np.stack(c, -1).astype(np.uint32)


def sample_poses(task, seed, episode_ids):
    """[n, nobj, 7] initial object poses of the given episode ids: the library's sampler (avsim_sample_poses) restated in numpy."""
    box, share = (np.asarray(x) for x in OBJECT_BOXES[task])
    ids = np.asarray(episode_ids, dtype=np.int64).astype(np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros((len(ids), len(share), 7))
    out[:, :, 3] = 1.0
    for o in range(len(share)):
        if 0 <= share[o] < o:
            out[:, o, :3] = out[:, share[o], :3]
            continue
        ctr = np.stack([ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32), np.full_like(ids, o), np.zeros_like(ids)], -1)
        x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
        u = (x[:, :3].astype(np.float64) + 0.5) * 2.0 ** -32
        lo, hi = box[o, :3], box[o, 3:]
        out[:, o, :3] = lo + (hi - lo) * u
    return out


class VecEnv(DeviceImageOps):
    """num_envs envs of one task on one GPU; see the module's docstring for the semantics.  The image calls on any tensor of the env's device
    -- decode_jpeg, encode_images, compose, compose_label, image_stats, prep_images, jitter_images, augment_images, resize_images -- and
    camera_poses / render_labels / point_cloud / voxel_grid / virtual_views on demand are images.DeviceImageOps's (images.ImageCalls on tensors)."""

    metadata = {"autoreset_mode": "NextStep", "render_modes": []}

    def __init__(self, task, num_arms, num_envs, max_episode_steps, device=None, cameras=(), depth_cameras=(), obs_format="lerobot",
                 seed=0, terminate_on_success=False, f64=False, options=None, observation_height=480, observation_width=640, pointcloud=None, voxels=None, views=None,
                 segmentation=None):
        import torch
        assert obs_format in ("lerobot", "gym"), obs_format
        assert all(c in CAMERAS for c in list(cameras) + list(depth_cameras)), "Invalid camera names"
        if voxels is not None and (list(cameras) or float((options or {}).get("render_cam_major", 0)) != 0):      # (before there is a handle to give back)
            raise ValueError("vec_env: voxels are refused together with the render_cam_major option (which `cameras` switch on): the grid reads env-major images")
        if views is not None and (list(cameras) or float((options or {}).get("render_cam_major", 0)) != 0):
            raise ValueError("vec_env: views are refused together with the render_cam_major option (which `cameras` switch on): the virtual views read env-major images")
        self.torch = torch
        self.task, self.num_arms, self.num_envs = task, num_arms, int(num_envs)
        self.max_episode_steps, self.terminate_on_success = int(max_episode_steps), bool(terminate_on_success)
        self.cameras, self.depth_cameras, self.obs_format = list(cameras), list(depth_cameras), obs_format
        self.observation_height, self.observation_width = int(observation_height), int(observation_width)
        if not torch.cuda.is_available():
            raise RuntimeError("vec_env: torch sees no GPU -- initialise torch's GPU before creating any other libavsim handle in this process")
        d = torch.device("cuda", device) if isinstance(device, int) else torch.device(device if device is not None else "cuda")
        self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        blob, self.manifest = load_blob(task, num_arms)
        vx = None
        if voxels is not None:          # checked before there is a handle to give back
            from . import pointcloud as pcspec, voxel as voxspec
            vx = dict(voxels)
            cams = list(vx["cameras"])
            assert all(c in CAMERAS for c in cams), "Invalid camera names"
            vx = {"cameras": cams, "ids": camera_ids(self.manifest, cams), "height": int(vx["height"]), "width": int(vx["width"]), "g": voxspec.grid_dims(vx["grid"]),
                  "bounds": np.ascontiguousarray(vx["bounds"], dtype=np.float32).reshape(-1), "colour": bool(vx.get("colour")),
                  "max_depth": float(pcspec.FAR_PLANE if vx.get("max_depth") is None else vx["max_depth"])}
            voxspec.check_voxel_grid(len(self.manifest["camera_names"]), vx["ids"], vx["height"], vx["width"], vx["bounds"], vx["max_depth"], vx["g"])
        vv = None
        if views is not None:           # likewise
            from . import pointcloud as pcspec, virtviews as vvspec
            vv = dict(views)
            cams = list(vv["cameras"])
            assert all(c in CAMERAS for c in cams), "Invalid camera names"
            vv = {"cameras": cams, "ids": camera_ids(self.manifest, cams), "height": int(vv["height"]), "width": int(vv["width"]),
                  "codes": np.array(vvspec.view_codes(vv.get("views", ["+z", "+x", "-x", "+y", "-y"])), dtype=np.int32), "size": np.array(vvspec.view_size(vv.get("size", 220)), dtype=np.int32),
                  "radius": int(vv.get("radius", 1)), "bounds": np.ascontiguousarray(vv["bounds"], dtype=np.float32).reshape(-1), "colour": bool(vv.get("colour", True)),
                  "max_depth": float(pcspec.FAR_PLANE if vv.get("max_depth") is None else vv["max_depth"])}
            vvspec.check_virtual_views(len(self.manifest["camera_names"]), vv["ids"], vv["height"], vv["width"], vv["bounds"], vv["max_depth"], vv["codes"], vv["size"], vv["radius"])
        sg = None
        if segmentation is not None:    # likewise
            from . import segment
            sg = dict(segmentation)
            cams = list(sg["cameras"])
            assert all(c in CAMERAS for c in cams), "Invalid camera names"
            kind = sg.get("kind", "class")
            table, names = self.label_table(kind) if isinstance(kind, str) else (np.ascontiguousarray(kind), None)
            sg = {"cameras": cams, "ids": camera_ids(self.manifest, cams), "height": int(sg["height"]), "width": int(sg["width"]), "table": table, "names": names}
            segment.check_labels(len(self.manifest["camera_names"]), len(self.manifest["geom_names"]), sg["ids"], sg["height"], sg["width"], table, None, depth=False)
        flags = _ffi.AVSIM_IO_DEVICE | (_ffi.AVSIM_F64_PHYSICS if f64 else 0)
        with torch.cuda.device(self.device):
            self.h = _ffi.Handle(blob, self.num_envs, self.device.index, flags)
        self.L, self.nj, self.nobj, self.max_reward = self.h.L, self.h.nj, self.h.nobj, self.h.max_reward
        self.num_joints = self.nj
        # the colour images as the gym facades draw them (env.py: shadows, 4 samples, smooth shading)
        options = {"render_shadows": 1, "render_samples": 4, "render_smooth": 1, **(options or {})}
        for k, v in options.items():
            self.h.check(self.L.avsim_set_option(self.h.h, k.encode(), float(v)))
        self._cam_major = int(float(options.get("render_cam_major", 0)) != 0)      # what voxel_grid's own colour render puts the option back to
        self._cam_ids, self._depth_ids = camera_ids(self.manifest, self.cameras), camera_ids(self.manifest, self.depth_cameras)
        if self.cameras:
            with open(os.path.join(MODEL_DIR, "visual_meshes.avv"), "rb") as f:
                lib = f.read()
            self.h.check(self.L.avsim_load_visual(self.h.h, lib, len(lib)))
            self.h.check(self.L.avsim_set_option(self.h.h, b"render_proxies", 0.0))
            self.h.check(self.L.avsim_set_option(self.h.h, b"render_cam_major", 1.0))     # every camera's batch contiguous
            self._cam_major = 1
        self._box = np.ascontiguousarray(OBJECT_BOXES[task][0], dtype=np.float64)
        self._share = np.ascontiguousarray(OBJECT_BOXES[task][1], dtype=np.int32)
        assert self._box.shape == (self.nobj, 6)
        self.seed = int(seed)
        self._log_capacity = 0
        self._stream = None
        # output buffers (overwritten by every call)
        N, dev, H, W = self.num_envs, self.device, self.observation_height, self.observation_width
        self._ap = torch.zeros((N, self.nj), dtype=torch.float64, device=dev)
        self._state = torch.zeros((N, self.nj), dtype=torch.float32, device=dev)
        self._reward = torch.zeros(N, dtype=torch.int32, device=dev)
        self._success = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._term = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._trunc = torch.zeros(N, dtype=torch.uint8, device=dev)
        self._id = torch.zeros(N, dtype=torch.int64, device=dev)
        self._elapsed = torch.zeros(N, dtype=torch.int32, device=dev)
        self._diag = torch.zeros((N, 4), dtype=torch.int32, device=dev)
        nc = len(self.cameras)
        if obs_format == "lerobot":
            self._img = torch.zeros((nc, N, 3, H, W), dtype=torch.float32, device=dev) if nc else None
        else:
            self._img = torch.zeros((nc, N, H, W, 3), dtype=torch.uint8, device=dev) if nc else None
        self._depth = torch.zeros((N, len(self.depth_cameras), H, W), dtype=torch.float32, device=dev) if self.depth_cameras else None
        self._pc = None
        if pointcloud is not None:      # a fixed-size world-frame cloud per env as an observation: its own cameras, size and depth buffer
            from . import pointcloud as pcspec
            pc = dict(pointcloud)
            cams = list(pc["cameras"])
            assert all(c in CAMERAS for c in cams), "Invalid camera names"
            ids = camera_ids(self.manifest, cams)
            ph, pw, P = int(pc["height"]), int(pc["width"]), int(pc["points"])
            b = np.ascontiguousarray(pc["bounds"], dtype=np.float32).reshape(-1)
            md = float(pcspec.FAR_PLANE if pc.get("max_depth") is None else pc["max_depth"])
            pcspec.check_point_cloud(len(self.manifest["camera_names"]), ids, ph, pw, b, md, P)
            self._pc = {"cameras": cams, "ids": ids, "height": ph, "width": pw, "bounds": b, "points": P, "max_depth": md, **self._drop_of(pc),
                        "labels": torch.zeros((N, len(cams), ph, pw), dtype=torch.uint8, device=dev) if pc.get("labels") else None,
                        "label": torch.zeros((N, P), dtype=torch.uint8, device=dev) if pc.get("labels") else None,
                        "depth": torch.zeros((N, len(cams), ph, pw), dtype=torch.float32, device=dev),
                        "xyz": torch.zeros((N, P, 3), dtype=torch.float32, device=dev), "index": torch.zeros((N, P), dtype=torch.int32, device=dev),
                        "count": torch.zeros((N, 2), dtype=torch.int32, device=dev)}
        self._vox = None
        if vx is not None:          # a dense world-frame grid per env as an observation: its own cameras, size, depth and colour buffers
            grid = torch.zeros((N,) + vx["g"] + (8,), dtype=torch.float32, device=dev)
            nc = len(vx["cameras"])
            self._vox = {**vx, **self._drop_of(voxels), "dims": np.array(vx["g"], dtype=np.int32), "depth": torch.zeros((N, nc, vx["height"], vx["width"]), dtype=torch.float32, device=dev),
                         "rgb": torch.zeros((N, nc, vx["height"], vx["width"], 3), dtype=torch.uint8, device=dev) if vx["colour"] else None,
                         "grid": grid, "view": grid.permute(0, 4, 1, 2, 3)}
        self._vv = None
        if vv is not None:          # RVT's orthographic images of the box per env as an observation: their own cameras, size, depth and colour buffers
            nc, vshape = len(vv["cameras"]), (N, len(vv["codes"]), int(vv["size"][0]), int(vv["size"][1]))
            out = torch.zeros(vshape + (8,), dtype=torch.float32, device=dev)
            self._vv = {**vv, **self._drop_of(views), "depth": torch.zeros((N, nc, vv["height"], vv["width"]), dtype=torch.float32, device=dev),
                        "rgb": torch.zeros((N, nc, vv["height"], vv["width"], 3), dtype=torch.uint8, device=dev) if vv["colour"] else None,
                        "out": out, "view": out.permute(0, 1, 4, 2, 3), "index": torch.zeros(vshape, dtype=torch.int32, device=dev)}
        self._seg = None
        if sg is not None:          # what every pixel shows as an observation: its own cameras, size and label buffer
            self._seg = {**sg, "labels": torch.zeros((N, len(sg["cameras"]), sg["height"], sg["width"]), dtype=torch.uint8, device=dev)}
            self.segmentation_classes = sg["names"]
        self._bind_stream()
        self._setup(self.seed, 0)

    # -- plumbing ----------------------------------------------------------------------------------
    def _setup(self, seed, log_capacity):
        self._bind_stream()
        self.seed, self._log_capacity = int(seed), int(log_capacity)
        self.h.check(self.L.avsim_episode_setup(self.h.h, self._box.ctypes.data, self._share.ctypes.data, self.seed & 0xFFFFFFFFFFFFFFFF,
                                                self.max_episode_steps, int(self.terminate_on_success), self._log_capacity))

    def _drop_of(self, option):
        """{"table", "drop"} of a pointcloud / voxels / views option: the class table and the flags of its "drop" names, None without any."""
        if not option.get("drop") and not option.get("labels"):
            return {"table": None, "drop": None}
        from . import segment
        table, names = self.label_table("class")
        return {"table": table, "drop": segment.drop_flags(option.get("drop"), names)}

    def _depth_of(self, o):
        """The depth buffer of a pointcloud / voxels / views option: avsim_render_depth's image, or -- with "drop" or "labels" -- avsim_render_labels's,
        the dropped classes at the far plane."""
        ids, nc = o["ids"].ctypes.data, len(o["cameras"])
        if o["table"] is None:
            self.h.check(self.L.avsim_render_depth(self.h.h, ids, nc, o["height"], o["width"], o["depth"].data_ptr()))
        else:
            self.h.check(self.L.avsim_render_labels(self.h.h, ids, nc, o["height"], o["width"], o["table"].ctypes.data, _ffi.ptr(o["drop"]), o["depth"].data_ptr(),
                                                    _ffi.ptr(o.get("labels"))))

    def _obs(self):
        L, h = self.L, self.h.h
        H, W = self.observation_height, self.observation_width
        if self.cameras:
            ids, nc = self._cam_ids.ctypes.data, len(self.cameras)
            if self.obs_format == "lerobot":
                self.h.check(L.avsim_render_rgb_f32(h, ids, nc, H, W, self._img.data_ptr()))
            else:
                self.h.check(L.avsim_render_rgb(h, ids, nc, H, W, self._img.data_ptr()))
        if self.depth_cameras:
            self.h.check(L.avsim_render_depth(h, self._depth_ids.ctypes.data, len(self.depth_cameras), H, W, self._depth.data_ptr()))
        if self.obs_format == "lerobot":
            self._state.copy_(self._ap)
            obs = {f"observation.images.{c}": self._img[i] for i, c in enumerate(self.cameras)}
            obs["observation.state"] = self._state
        else:
            obs = {"pixels": {c: self._img[i] for i, c in enumerate(self.cameras)}, "agent_pos": self._ap}
        if self.depth_cameras:
            obs["depth"] = {c: self._depth[:, i] for i, c in enumerate(self.depth_cameras)}
        if self._pc is not None:
            pc = self._pc
            ids, nc = pc["ids"].ctypes.data, len(pc["cameras"])
            self._depth_of(pc)
            self.h.check(L.avsim_point_cloud(h, ids, nc, pc["height"], pc["width"], pc["depth"].data_ptr(), pc["bounds"].ctypes.data, pc["max_depth"], pc["points"],
                                             pc["xyz"].data_ptr(), pc["index"].data_ptr(), pc["count"].data_ptr()))
            if pc["labels"] is not None:        # the class image gathered at the points' pixels
                self.torch.gather(pc["labels"].view(self.num_envs, -1), 1, pc["index"].clamp(min=0).long(), out=pc["label"])
                pc["label"].masked_fill_(pc["index"] < 0, 255)
            obs["observation.pointcloud" if self.obs_format == "lerobot" else "pointcloud"] = pc["xyz"]
        if self._vox is not None:
            vx = self._vox
            ids, nc = vx["ids"].ctypes.data, len(vx["cameras"])
            self._depth_of(vx)
            if vx["rgb"] is not None:
                self.h.check(L.avsim_render_rgb(h, ids, nc, vx["height"], vx["width"], vx["rgb"].data_ptr()))
            self.h.check(L.avsim_voxel_grid(h, ids, nc, vx["height"], vx["width"], vx["depth"].data_ptr(), _ffi.ptr(vx["rgb"]), vx["bounds"].ctypes.data, vx["max_depth"],
                                            vx["dims"].ctypes.data, vx["grid"].data_ptr()))
            obs["observation.voxels" if self.obs_format == "lerobot" else "voxels"] = vx["view"]
        if self._vv is not None:
            vv = self._vv
            ids, nc = vv["ids"].ctypes.data, len(vv["cameras"])
            self._depth_of(vv)
            if vv["rgb"] is not None:
                self.h.check(L.avsim_render_rgb(h, ids, nc, vv["height"], vv["width"], vv["rgb"].data_ptr()))
            self.h.check(L.avsim_virtual_views(h, ids, nc, vv["height"], vv["width"], vv["depth"].data_ptr(), _ffi.ptr(vv["rgb"]), vv["bounds"].ctypes.data, vv["max_depth"],
                                               vv["codes"].ctypes.data, len(vv["codes"]), vv["size"].ctypes.data, vv["radius"], vv["out"].data_ptr(), vv["index"].data_ptr()))
            obs["observation.virtual_views" if self.obs_format == "lerobot" else "virtual_views"] = vv["view"]
        if self._seg is not None:
            sg = self._seg
            self.h.check(L.avsim_render_labels(h, sg["ids"].ctypes.data, len(sg["cameras"]), sg["height"], sg["width"], sg["table"].ctypes.data, None, None, sg["labels"].data_ptr()))
            if self.obs_format == "lerobot":
                obs["observation.segmentation"] = sg["labels"]
            else:
                obs["segmentation"] = {c: sg["labels"][:, i] for i, c in enumerate(sg["cameras"])}
        return obs

    def _pc_info(self, info):
        if self._pc is not None:
            info["pointcloud_count"], info["pointcloud_index"] = self._pc["count"], self._pc["index"]
            if self._pc["label"] is not None:
                info["pointcloud_label"] = self._pc["label"]
        if self._vv is not None:
            info["virtual_views_index"] = self._vv["index"]
        return info

    # -- gym API -------------------------------------------------------------------------------------
    def reset(self, seed=None, options=None):
        """seed: restart the episode ids at 0 under this seed (and drop the records); options={"reset_mask": bool [N]}: only those envs
        start a new episode, the others keep theirs."""
        self._bind_stream()
        if seed is not None:
            self._setup(seed, self._log_capacity)
        mask = (options or {}).get("reset_mask")
        if mask is not None:
            mask = self.torch.as_tensor(mask, device=self.device).to(self.torch.uint8).contiguous()
            assert mask.shape == (self.num_envs,)
        self.h.check(self.L.avsim_episode_reset(self.h.h, _ffi.ptr(mask), self._ap.data_ptr(), self._id.data_ptr()))
        for t in (self._elapsed, self._success, self._reward, self._term, self._trunc):      # (the envs that keep their episode keep their last step's)
            t.masked_fill_(mask.bool(), 0) if mask is not None else t.zero_()
        return self._obs(), self._pc_info({"episode_id": self._id, "elapsed_steps": self._elapsed, "is_success": self._success.view(self.torch.bool)})

    def step(self, action):
        torch = self.torch
        self._bind_stream()
        assert isinstance(action, torch.Tensor) and action.dtype == torch.float32 and action.device == self.device, \
            "step(action): a float32 tensor on the env's device"
        assert tuple(action.shape) == (self.num_envs, self.nj), f"action shape {tuple(action.shape)} != {(self.num_envs, self.nj)}"
        a = action.contiguous()
        self.h.check(self.L.avsim_episode_step(self.h.h, a.data_ptr(), SIM_PHYSICS_ENV_STEP_RATIO, self._ap.data_ptr(), self._reward.data_ptr(),
                                               self._success.data_ptr(), self._term.data_ptr(), self._trunc.data_ptr(), self._id.data_ptr(),
                                               self._elapsed.data_ptr()))
        self.h.check(self.L.avsim_get_diag(self.h.h, self._diag.data_ptr()))
        obs = self._obs()
        diverged = ((self._diag[:, 3] & 1) != 0) & (self._elapsed > 0)       # (an env that starts an episode in this call has not diverged)
        info = self._pc_info({"is_success": self._success.view(torch.bool), "episode_id": self._id, "elapsed_steps": self._elapsed, "diverged": diverged})
        return obs, self._reward, self._term.view(torch.bool), self._trunc.view(torch.bool), info

    # -- episode records -----------------------------------------------------------------------------
    def start_log(self, log_capacity, seed=None):
        """Restart the episode ids at 0 (under `seed`, default the current one) and keep the records of ids [0, log_capacity)."""
        self._setup(self.seed if seed is None else seed, log_capacity)

    def episode_count(self):
        """(episodes started, episodes finished) since the last seed / start_log; synchronises."""
        c = np.zeros(2, dtype=np.int64)
        self.h.check(self.L.avsim_episode_count(self.h.h, c.ctypes.data))
        return int(c[0]), int(c[1])

    def episode_log(self, n):
        """Records of episode ids [0, n) as numpy arrays (length 0: not finished); synchronises."""
        ret, length = np.zeros(n), np.zeros(n, dtype=np.int32)
        mr, su = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        obj = np.zeros((n, self.nobj, 7))
        self.h.check(self.L.avsim_episode_log(self.h.h, n, ret.ctypes.data, length.ctypes.data, mr.ctypes.data, su.ctypes.data, obj.ctypes.data))
        return {"return": ret, "length": length, "max_reward": mr, "success": su.astype(bool), "initial_object_poses": obj}

    def sample_poses(self, episode_ids, seed=None):
        """The library's initial poses [n, nobj, 7] of the given episode ids (under `seed`, default the env's); synchronises."""
        ids = np.ascontiguousarray(episode_ids, dtype=np.int64)
        out = np.zeros((len(ids), self.nobj, 7))
        if len(ids):
            t_ids = self.torch.from_numpy(ids).to(self.device)
            t_out = self.torch.zeros((len(ids), self.nobj, 7), dtype=self.torch.float64, device=self.device)
            self._bind_stream()
            self.h.check(self.L.avsim_sample_poses(self.h.h, (self.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF, len(ids),
                                                   t_ids.data_ptr(), t_out.data_ptr()))
            out = t_out.cpu().numpy()
        return out

    def jpeg_stride(self, quality=90):
        """Bytes encode_jpeg reserves per stream by default: half the raw frame, never more than the worst case (avsim_jpeg_bound).  A
        rendered 480 x 640 frame takes 31 KB at quality 90 and 95 KB at 100."""
        return default_stride(self.L, self.observation_height, self.observation_width, 2)

    def encode_jpeg(self, camera, envs=None, quality=90, out=None, out_len=None):
        """JPEG streams of `camera`'s CURRENT observation (the images the last reset / step returned), encoded on the device from the
        observation buffer itself (lerobot format: the float32 planes, gym format: the u8 pixels; both give the same bytes).  envs: None =
        all, an int n = the first n envs, or an int32 index tensor on the env's device (values outside [0, num_envs) are clamped).
        -> (out uint8 [n, stride], out_len int32 [n]) on the device; stream i is out[i, :out_len[i]], and one with out_len[i] > stride did
        not fit (pass a larger `out`; the default stride is jpeg_stride()).  out / out_len: buffers to write into.  Does not synchronise."""
        torch = self.torch
        self._bind_stream()
        if camera not in self.cameras:
            raise ValueError(f"encode_jpeg: the env does not render {camera!r} (cameras: {self.cameras})")
        index = None
        if envs is None:
            n = self.num_envs
        elif isinstance(envs, int):
            n = envs
            if not 0 <= n <= self.num_envs:
                raise ValueError(f"encode_jpeg: envs={n} of {self.num_envs}")
        else:
            assert isinstance(envs, torch.Tensor) and envs.dtype == torch.int32 and envs.device == self.device and envs.ndim == 1, \
                "encode_jpeg(envs=...): an int32 index tensor on the env's device"
            index = envs.clamp(0, self.num_envs - 1).contiguous()
            n = int(index.shape[0])
        return self._encode(self._img[self.cameras.index(camera)], 1 if self.obs_format == "lerobot" else 0, index, n, self.observation_height,
                            self.observation_width, quality, out, out_len)

    def camera_images(self, camera):
        """The buffer that holds `camera`'s current observation of all envs: float32 [N, 3, H, W] (lerobot) or uint8 [N, H, W, 3] (gym)."""
        if camera not in self.cameras:
            raise ValueError(f"the env does not render {camera!r} (cameras: {self.cameras})")
        return self._img[self.cameras.index(camera)]

    def check_render_overflow(self):
        """Overflow flags of the last colour render (bit 0 triangle records, bit 1 tile lists; 0 = complete images): warns when set.
        Synchronises, so it is read once at the end of an evaluation rather than per step."""
        if not self.cameras:
            return 0
        info = np.zeros(4, dtype=np.int32)
        self.h.check(self.L.avsim_visual_info(self.h.h, info.ctypes.data))
        if info[2]:
            warnings.warn(f"vector env: a view ran out of triangle records / tile-list entries (flags {int(info[2])}): triangles were "
                          "dropped from some images", RuntimeWarning, stacklevel=2)
        return int(info[2])


def make_vec(env_id, num_envs, max_episode_steps, device=None, cameras=None, depth_cameras=(), obs_format="lerobot", seed=0,
             terminate_on_success=False, f64=False, options=None, observation_height=None, observation_width=None, pointcloud=None, voxels=None, views=None,
             segmentation=None):
    """A VecEnv of a registry id (env.ENVS); cameras default to the registry's, the image size to its 480 x 640.  pointcloud, voxels, views, segmentation: VecEnv's."""
    spec = ENVS[env_id]
    return VecEnv(_TASK_OF_CLASS[spec["env"]], spec["num_arms"], num_envs, max_episode_steps, device=device,
                  cameras=spec["cameras"] if cameras is None else cameras, depth_cameras=depth_cameras, obs_format=obs_format, seed=seed,
                  terminate_on_success=terminate_on_success, f64=f64, options=options,
                  observation_height=spec["observation_height"] if observation_height is None else observation_height,
                  observation_width=spec["observation_width"] if observation_width is None else observation_width, pointcloud=pointcloud, voxels=voxels, views=views,
                  segmentation=segmentation)
