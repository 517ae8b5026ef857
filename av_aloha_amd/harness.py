"""Rollout and recording harnesses: the counterparts of eval_scripts/eval.py and data_collection_scripts/record_sim_episodes.py
(SURVEY 8f ranks 1-2), host glue over the environments of env.py / sim_env.py.

* `preprocess_observation` (eval.py:23-66): gym observation -> LeRobot-style tensors (`observation.images.<cam>` float32 CHW in
  [0, 1] resized to 480 x 640, `observation.state` float32 with a leading batch axis).
* `rollout` (eval.py:96-124): reset / select_action / step loop for `num_episodes` x `episode_len`, frames of zed_cam_left when
  the env returns pixels, plus the success / return bookkeeping the reference leaves out.  Works on one env (reference shapes)
  and on a batch (`num_envs > 1`).
* `evaluate_vec`: the same evaluation on the device-resident vector env (vec_env.py): per-env episodes, NEXT_STEP autoreset, one
  record per episode id, no host round trip per step; optionally the first episodes' videos (eval.py:118-128) as Motion-JPEG AVI files
  whose frames are encoded on the device (jpeg.py, mjpeg.py).
* `record_episode` / `save_episode` / `load_episode` (record_sim_episodes.py:83-128, :155-212): a scripted Cartesian action
  sequence replaces the VR headset; the episode holds T = len(actions) + 1 time steps with `/observations/qpos` (T, 21),
  `/observations/qvel` (T, 21), `/observations/all_qpos` (T, nq), `/action` (T, 21: the joint-space command with
  normalised grippers, i.e. obs['control']) as float32, `/observations/images/<cam>` uint8 (T, H, W, 3) for the env's cameras
  and the attribute sim = True.  Written as HDF5 either way: through h5py when it is importable, otherwise through the
  package's own minimal writer (av_aloha_amd/hdf5min.py: same groups, names, dtypes, image chunking (1, H, W, 3) and attribute, in
  the structures libhdf5 writes by default); `load_episode` reads both, and the older .npz files.
* `replay_episode` (gym_guided_vision/scripts/replay_sim_episode.py:221-262): set_qpos through `/observations/all_qpos`.
* `rerender_episode` / `rerender_dataset` (gym_guided_vision/scripts/replay_sim_episode.py:47-113): how the reference makes its
  per-camera-configuration training sets -- a recorded episode's full states are put back frame by frame (`set_qpos`), the gym env
  of the wanted camera configuration renders its registered cameras (`get_obs()["pixels"]`), and a new HDF5 is written with those
  images next to the recorded qpos / qvel / action (the first 14 columns for a 2-arm env).  Here the T frames of an episode are T
  envs of ONE batched handle: one set_qpos, one render call per chunk of frames.
"""
from __future__ import annotations

import os

import numpy as np

IMAGE_SIZE = (480, 640)        # eval.py:20 RESIZE


def preprocess_observation(observations: dict) -> dict:
    import torch
    import torch.nn.functional as F
    out = {}
    if "pixels" in observations and observations["pixels"] is not None:
        px = observations["pixels"]
        imgs = {f"observation.images.{k}": v for k, v in px.items()} if isinstance(px, dict) else {"observation.image": px}
        for key, img in imgs.items():
            t = torch.from_numpy(np.ascontiguousarray(img).copy())
            if t.ndim == 3:
                t = t.unsqueeze(0)
            _, h, w, c = t.shape
            assert c < h and c < w, f"expect channel last images, but instead got {tuple(t.shape)}"
            assert t.dtype == torch.uint8, f"expect torch.uint8, but instead {t.dtype}"
            t = t.permute(0, 3, 1, 2).contiguous().to(torch.float32) / 255
            if (h, w) != IMAGE_SIZE:
                t = F.interpolate(t, size=IMAGE_SIZE, mode="bilinear", antialias=True, align_corners=False)
            out[key] = t
    if "environment_state" in observations:
        out["observation.environment_state"] = torch.from_numpy(np.asarray(observations["environment_state"])).float()
    state = torch.from_numpy(np.asarray(observations["agent_pos"])).float()
    out["observation.state"] = state.unsqueeze(0) if state.ndim == 1 else state
    return out


def rollout(env, select_action, episode_len: int, num_episodes: int = 1, reset_policy=None, video_path: str | None = None, video_quality: int = 90):
    """select_action(dict of tensors) -> array-like (batch, action_dim).  Returns per-episode dicts with 'return' (sum of the
    rewards), 'success' (is_success seen at any step), 'max_reward' and the captured 'frames'.  video_path: a format string taking the
    episode number ("outputs/rollout_{}.avi", eval.py:123); the episode's zed_cam_left frames are then also encoded on the device
    (BatchedSim.encode_jpeg) and written as a Motion-JPEG AVI at 50 frames per second (eval.py:128); of a batched env, env 0's frames."""
    results = []
    batched = getattr(env, "num_envs", 1) > 1
    for episode in range(num_episodes):
        if reset_policy is not None:
            reset_policy()
        observation, info = env.reset()
        ret = 0
        success = np.zeros(getattr(env, "num_envs", 1), dtype=bool)
        frames = []
        for _ in range(episode_len):
            action = np.asarray(select_action(preprocess_observation(observation)))
            assert action.ndim == 2, "Action dimensions should be (batch, action_dim)"
            observation, reward, terminated, truncated, info = env.step(action if batched else action[0])
            ret = ret + np.asarray(reward)
            success |= np.asarray(info["is_success"], dtype=bool).reshape(-1)
            px = observation.get("pixels") or {}
            if "zed_cam_left" in px:
                frames.append(px["zed_cam_left"])
        if video_path is not None and frames:
            from .mjpeg import AviWriter
            path = video_path.format(episode)
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            stack = np.stack([f[0] if batched else f for f in frames])
            with AviWriter(path, stack.shape[2], stack.shape[1], fps=50) as w:
                for stream in env.sim.encode_jpeg(stack, quality=video_quality):
                    w.add(stream)
        results.append({"return": ret, "success": success if batched else bool(success[0]), "max_reward": env.max_reward, "frames": frames})
    return results


class _VideoRecorder:
    """The first `episodes` episodes of a vector env as Motion-JPEG files: every step's frames of envs [0, episodes) are encoded on the
    device into a chunk of buffers next to their episode ids; a full chunk comes to the host in one copy and is split over the files."""

    def __init__(self, env, video_dir, camera, episodes, quality, fps):
        from .mjpeg import AviWriter
        import torch
        self.env, self.k, self.quality, self.camera = env, int(episodes), int(quality), camera
        os.makedirs(video_dir, exist_ok=True)
        H, W = env.observation_height, env.observation_width
        self.writers = [AviWriter(os.path.join(video_dir, f"rollout_{i}.avi"), W, H, fps=fps) for i in range(self.k)]
        self.open = [True] * self.k
        stride = env.jpeg_stride(quality)
        self.chunk = max(1, min(64, (256 << 20) // (stride * self.k)))
        self.buf = torch.empty((self.chunk, self.k, stride), dtype=torch.uint8, device=env.device)
        self.len = torch.zeros((self.chunk, self.k), dtype=torch.int32, device=env.device)
        self.ids = torch.zeros((self.chunk, self.k), dtype=torch.int64, device=env.device)
        self.fill = 0

    @property
    def active(self):
        return any(self.open)

    def add(self, info):
        """After a step: its frames of envs [0, k)."""
        c = self.fill
        self.env.encode_jpeg(self.camera, envs=self.k, quality=self.quality, out=self.buf[c], out_len=self.len[c])
        self.ids[c].copy_(info["episode_id"][:self.k])
        self.fill += 1
        if self.fill == self.chunk:
            self.flush()

    def flush(self):
        n, self.fill = self.fill, 0
        if n == 0:
            return
        ln, ids = self.len[:n].cpu().numpy(), self.ids[:n].cpu().numpy()          # (these copies wait for the stream)
        stride = self.buf.shape[2]
        keep = (ids == np.arange(self.k)[None]) & np.asarray(self.open)[None]
        if (ln[keep] > stride).any():
            raise RuntimeError(f"evaluate_vec: a frame's JPEG stream ({int(ln[keep].max())} B) is longer than the {stride} B reserved for it")
        width = int(ln[keep].max()) if keep.any() else 0
        data = self.buf[:n, :, :width].cpu().numpy()                                # only as many bytes per stream as the longest one has
        for c in range(n):
            for e in range(self.k):
                if not self.open[e]:
                    continue
                if keep[c, e]:
                    self.writers[e].add(data[c, e, :ln[c, e]].tobytes())
                else:                                                               # env e went on to a later episode: its video is complete
                    self.writers[e].close()
                    self.open[e] = False

    def close(self, ok=True):
        try:
            if ok:
                self.flush()
        finally:
            for e, w in enumerate(self.writers):
                if self.open[e]:
                    w.close() if ok else w.abort()
                    self.open[e] = False


class _GridRecorder:
    """One Motion-JPEG file of a vector env's batch: every step's frames of envs [0, k) are shrunk into the cells of a grid, labelled with the
    envs' episode ids (read on the device) and encoded there, into a chunk of buffers that comes to the host in one copy."""

    def __init__(self, env, path, camera, k, cols, cell, quality, fps):
        from .compose import layout_grid
        from .images import default_stride
        from .mjpeg import AviWriter
        import torch
        self.env, self.k, self.quality = env, int(k), int(quality)
        self.src = env.camera_images(camera)
        cell_h, cell_w = int(cell[0]), int(cell[1])
        rows, CH, CW = layout_grid(self.k, cell_h, cell_w, cols)
        self.places = np.array([(0, e, x0, y0, w, h) for e, (x0, y0, w, h) in enumerate(rows)], dtype=np.int32)
        self.where = np.array([(0, x0 + 2, y0 + 2, max(1, cell_h // 60)) for x0, y0, _, _ in rows], dtype=np.int32)
        self.canvas = torch.zeros((1, CH, CW, 3), dtype=torch.uint8, device=env.device)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.writer = AviWriter(path, CW, CH, fps=fps)
        stride = default_stride(env.L, CH, CW, 2)
        self.chunk = max(1, min(64, (256 << 20) // stride))
        self.buf = torch.empty((self.chunk, 1, stride), dtype=torch.uint8, device=env.device)
        self.len = torch.zeros((self.chunk, 1), dtype=torch.int32, device=env.device)
        self.ids = torch.zeros(self.k, dtype=torch.int64, device=env.device)
        self.fill = 0

    def add(self, info):
        """After a step: one frame."""
        env, c = self.env, self.fill
        env.compose(self.src, self.places, out=self.canvas, clear=0)
        self.ids.copy_(info["episode_id"][:self.k])
        env.compose_label(self.canvas, self.where, "", self.ids, 0xFFFFFF)
        env.encode_images(self.canvas, self.quality, out=self.buf[c], out_len=self.len[c])
        self.fill += 1
        if self.fill == self.chunk:
            self.flush()

    def flush(self):
        n, self.fill = self.fill, 0
        if n == 0:
            return
        ln = self.len[:n, 0].cpu().numpy()                       # (this copy waits for the stream)
        stride = self.buf.shape[2]
        if (ln > stride).any():
            raise RuntimeError(f"evaluate_vec: a grid frame's JPEG stream ({int(ln.max())} B) is longer than the {stride} B reserved for it")
        data = self.buf[:n, 0, :int(ln.max())].cpu().numpy()
        for c in range(n):
            self.writer.add(data[c, :ln[c]].tobytes())

    def close(self, ok=True):
        try:
            if ok:
                self.flush()
        finally:
            self.writer.close() if ok else self.writer.abort()


def evaluate_vec(env, select_action, num_episodes: int, seed: int | None = None, video_dir: str | None = None, video_camera: str | None = None,
                 video_episodes: int = 0, video_quality: int = 90, video_fps: float = 50, grid_video: str | None = None, grid_envs: int = 0,
                 grid_cols: int | None = None, grid_cell=(120, 160), grid_quality: int = 90) -> list:
    """Policy evaluation on a device-resident vector env (vec_env.make_vec): the episode ids restart at 0 and the env is stepped until
    the episodes with ids [0, num_episodes) have all finished; envs go on to later ids by themselves (NEXT_STEP autoreset).
    select_action(obs, info) -> float32 [N, nj] tensor on the env's device; info["episode_id"] changing marks an env's new episode.
    The host reads the episode counter once per max_episode_steps calls.  Returns one dict per id: 'episode_id', 'return', 'length',
    'max_reward', 'success', 'initial_object_poses'.

    Videos (eval.py:96-126 keeps zed_cam_left's frames and writes rollout_<i>.mp4): with video_dir and video_episodes = k > 0 the episodes
    with ids 0 .. k-1 -- the first episodes of envs 0 .. k-1 -- are written to <video_dir>/rollout_<id>.avi (Motion-JPEG, mjpeg.py), one
    frame per step call of the episode (the observation the call returned; the reset observation is not a frame), `length` frames in all.
    video_camera defaults to zed_cam_left when the env renders it, else to its first camera.  The frames are encoded on the device
    (VecEnv.encode_jpeg) into buffers that hold a chunk of calls and come to the host once per chunk -- that copy waits for the stream,
    the steps in between do not; recording stops when those episodes are over.  The records are the same with and without video.
    ValueError: video_episodes > env.num_envs, or a camera the env does not render.

    The batch at a glance: with grid_video (a path) and grid_envs = k > 0 ONE file is written whose every frame -- one per step call, until the
    evaluation ends -- holds video_camera's observation of envs 0 .. k-1, shrunk to grid_cell = (height, width) and laid out row by row
    (compose.layout_grid; grid_cols columns, default ceil(sqrt(k))), each cell labelled with its env's current episode id.  Composed
    (VecEnv.compose / compose_label, the id read from the device tensor) and encoded on the device, a chunk of frames per copy to the host.
    ValueError: grid_envs > env.num_envs, or a camera the env does not render."""
    video = grid = None
    if grid_video is not None and grid_envs > 0:
        if grid_envs > env.num_envs:
            raise ValueError(f"evaluate_vec: grid_envs={grid_envs} > num_envs={env.num_envs}")
        if video_camera is None:
            video_camera = "zed_cam_left" if "zed_cam_left" in env.cameras else (env.cameras[0] if env.cameras else None)
        if video_camera not in env.cameras:
            raise ValueError(f"evaluate_vec: the env does not render {video_camera!r} (cameras: {list(env.cameras)})")
    if video_dir is not None and video_episodes > 0:
        if video_episodes > env.num_envs:
            raise ValueError(f"evaluate_vec: video_episodes={video_episodes} > num_envs={env.num_envs} (the recorded episodes are the first episodes of envs 0 .. k-1)")
        if video_camera is None:
            video_camera = "zed_cam_left" if "zed_cam_left" in env.cameras else (env.cameras[0] if env.cameras else None)
        if video_camera not in env.cameras:
            raise ValueError(f"evaluate_vec: the env does not render {video_camera!r} (cameras: {list(env.cameras)})")
    env.start_log(num_episodes, seed=seed)
    observation, info = env.reset()
    if video_dir is not None and video_episodes > 0:
        video = _VideoRecorder(env, video_dir, video_camera, video_episodes, video_quality, video_fps)
    if grid_video is not None and grid_envs > 0:
        grid = _GridRecorder(env, grid_video, video_camera, grid_envs, grid_cols, grid_cell, grid_quality, video_fps)
    calls = 0
    try:
        while True:
            observation, reward, terminated, truncated, info = env.step(select_action(observation, info))
            calls += 1
            if video is not None and video.active:
                video.add(info)
            if grid is not None:
                grid.add(info)
            if calls % env.max_episode_steps == 0 and env.episode_count()[1] >= num_episodes:
                log = env.episode_log(num_episodes)
                if (log["length"] > 0).all():
                    break
    except BaseException:
        if video is not None:
            video.close(ok=False)
        if grid is not None:
            grid.close(ok=False)
        raise
    if video is not None:
        video.close()
    if grid is not None:
        grid.close()
    env.check_render_overflow()
    return [{"episode_id": i, "return": float(log["return"][i]), "length": int(log["length"][i]), "max_reward": int(log["max_reward"][i]),
             "success": bool(log["success"][i]), "initial_object_poses": log["initial_object_poses"][i]} for i in range(num_episodes)]


def make_preprocessor(venv, stats, crop=None, resize=None, resize_mode="stretch", antialias=True):
    """A function obs -> the policy's input for a VecEnv, with the numbers training used: dataset.TrainingBatches(crop_mode="center")'s.
    stats: CompressedDataset.stats()'s (dataset.load_stats'); crop = (h, w): the centred box (None: the whole image).  The function reads
    the env's own image buffers (VecEnv.camera_images, either observation format) through VecEnv.prep_images with
    imgprep.normalise_lut(stats) -- the bits of imgprep.prep_reference -- and normalises the state as (x - mean) / std in float32; it returns
    {"observation.images.<cam>": float32 [N, 3, h, w], "observation.state": float32 [N, D]} on the env's device and does not synchronise:
    evaluate_vec(venv, lambda obs, info: policy(pre(obs)), ...).
    resize = (oh, ow): the centred box is the source region of VecEnv.resize_images (avsim_image_resize) instead, resize_mode "stretch" or
    "pad" and antialias as in dataset.TrainingBatches(crop_mode="center", resize=...), whose numbers these are -- the bits of
    imgresize.resize_reference; the images are float32 [N, 3, oh, ow]."""
    import torch
    from . import imgprep, imgresize
    H, W = venv.observation_height, venv.observation_width
    h, w = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
    if not (1 <= h <= H and 1 <= w <= W):
        raise ValueError(f"crop {(h, w)} does not fit the env's {H} x {W} images")
    x0, y0 = imgprep.center_box((H, W), (h, w))
    box = np.tile(np.array([[x0, y0, 0]], dtype=np.int32), (venv.num_envs, 1))
    luts, mean_std = {}, {}
    if resize is not None:
        resize = (int(resize[0]), int(resize[1]))
        src_box, dst = imgresize.boxes(box, (h, w), resize, resize_mode)
        imgresize.check_resize((venv.num_envs, H, W), src_box, dst, None, resize)
    for c in venv.cameras:
        st = stats[f"observation.images.{c}"]
        mean_std[c] = (st["mean"], st["std"])
        luts[c] = torch.from_numpy(np.ascontiguousarray(imgprep.normalise_lut(st["mean"], st["std"]), dtype=np.float32).reshape(1, 3, 256)).to(venv.device)
    mean = torch.from_numpy(np.asarray(stats["observation.state"]["mean"], dtype=np.float32)).to(venv.device)
    std = torch.from_numpy(np.asarray(stats["observation.state"]["std"], dtype=np.float32)).to(venv.device)

    def pre(obs):
        state = obs["observation.state"] if "observation.state" in obs else obs["agent_pos"].to(torch.float32)
        out = {"observation.state": (state - mean) / std}
        for c in venv.cameras:
            if resize is not None:
                out[f"observation.images.{c}"] = venv.resize_images(venv.camera_images(c), src_box, dst, resize, antialias, mean=mean_std[c][0], std=mean_std[c][1])
            else:
                out[f"observation.images.{c}"] = venv.prep_images(venv.camera_images(c), luts[c], box, (h, w))
        return out

    return pre


def chunked_policy(venv, predict_chunk, chunk_size, ensemble=None, n_action_steps=None, first=0, stats=None, predict="when_needed", observe=None):
    """(select_action, executor) for evaluate_vec and a policy that predicts action CHUNKS (ACT, diffusion policies trained by
    dataset.TrainingBatches(chunk_size=...)): predict_chunk(obs, info) -> float32 [N, chunk_size, nj] on the env's device, normalised when
    `stats` (CompressedDataset.stats()'s) are given.  The executor (chunks.ActionChunks on venv) keeps the state PER ENV and starts an env's
    state anew when its episode does (a new info["episode_id"] or elapsed_steps 0), which a policy's own select_action with one queue or one
    ensembler for the batch does not: that is only right while all envs' episodes are in phase.
    ensemble = a coefficient (ACT's 0.01): LeRobot's temporal ensembling; predict_chunk runs in every call and nothing synchronises.
    ensemble None: a queue of n_action_steps (default chunk_size) rows from row `first` (a diffusion policy: n_obs_steps - 1, with `observe`).  predict =
    "when_needed": predict_chunk runs, for the whole batch, only in the calls where some env needs a chunk; select_action reads the executor's
    4-byte `any` flag to know -- the ONE synchronisation per call of this function.  predict = "always": it runs in every call, the envs
    that need no chunk ignore theirs, and nothing synchronises.  Neither setting can starve an env (executor.starved() stays 0).
    An evaluation's first call sees elapsed_steps 0 everywhere and so starts every env afresh; select_action cannot check that without a
    synchronisation and does not try: call executor.reset() before evaluate_vec when the executor has run before -- the explicit form of it.
    observe: a callable (obs, info) -> obs', run in EVERY call, before the decision whether to predict; predict_chunk receives its result.
    history_preprocessor's is the one for a policy with n_obs_steps > 1, whose history must see every observation although the policy itself
    is skipped in most calls.  None: predict_chunk receives the env's observation."""
    from .chunks import ActionChunks
    if predict not in ("when_needed", "always"):
        raise ValueError(f"predict {predict!r}: 'when_needed' or 'always'")
    executor = ActionChunks(venv, chunk_size, None, ensemble, n_action_steps, first, stats)
    ask = ensemble is None and predict == "when_needed"

    def select_action(obs, info):
        if observe is not None:
            obs = observe(obs, info)
        if ask:
            _, flag = executor.need(info)
            chunks = predict_chunk(obs, info) if int(flag.item()) else None          # (.item() waits for the stream)
        else:
            chunks = predict_chunk(obs, info)
        return executor.step(chunks, info)

    return select_action, executor


def history_preprocessor(venv, stats, crop=None, n_obs_steps=2, resize=None):
    """(observe, history) for chunked_policy(..., observe=observe) and a policy that reads n_obs_steps observations: history is an
    obshist.ObsHistory on venv with make_preprocessor's numbers (stats: CompressedDataset.stats()'s; crop = (h, w): the centred box), kept PER
    ENV -- an env that starts a new episode starts with n_obs_steps copies of its reset frame --, and observe(obs, info) pushes the env's
    observation and returns {"observation.state": float32 [N, K, D], "observation.images.<cam>": float32 [N, K, 3, h, w]}, slot K-1 the
    newest: what dataset.TrainingBatches(n_obs_steps=K, crop_mode="center") trains on.  Nothing synchronises.  Call history.reset() before
    evaluate_vec when the history has run before (chunked_policy's docstring says why).
    resize: not built -- the observation-history kernel keeps the crop's pixel grid; anything but None raises ValueError."""
    from .obshist import ObsHistory
    if resize is not None:
        raise ValueError("history_preprocessor: resize is not supported with observation histories (make_preprocessor has it)")
    H, W = venv.observation_height, venv.observation_width
    if crop is not None and not (1 <= int(crop[0]) <= H and 1 <= int(crop[1]) <= W):
        raise ValueError(f"crop {tuple(crop)} does not fit the env's {H} x {W} images")
    history = ObsHistory(venv, n_obs_steps, stats=stats, crop=crop)
    return history.push, history


def record_episode(env, actions23) -> dict:
    """Steps a Cartesian-action env (av_aloha_amd.sim_env) through `actions23` [T-1, 23] and returns the episode arrays."""
    ts = env.get_obs()
    steps = [ts]
    for a in np.asarray(actions23, dtype=np.float64):
        ts, _, _, _, _ = env.step(a)
        steps.append(ts)
    stack = lambda f: np.stack([np.asarray(f(s)) for s in steps]).astype(np.float32)
    data = {"/observations/qpos": stack(lambda s: s["joints"]["position"]), "/observations/qvel": stack(lambda s: s["joints"]["velocity"]),
            "/observations/all_qpos": stack(lambda s: s["qpos"]), "/action": stack(lambda s: s["control"])}
    for cam in steps[0].get("images", {}):                     # record_sim_episodes.py:197-200: uint8 (T, H, W, 3) per camera
        data[f"/observations/images/{cam}"] = np.stack([s["images"][cam] for s in steps])
    return data


def _image_bytes_per_step(cameras) -> int:
    """u8 bytes of one env's images per time step in the Cartesian env's sizes (sim_env.py:187-203)."""
    return sum(720 * 1440 * 3 if c == "zed_cam" else 480 * 640 * 3 for c in cameras)


def record_scripted(task_name: str, num_episodes: int, cameras=(), seed: int | None = None, device: int = 0, only_success: bool = False,
                    image_budget_bytes: int = 8 << 30, keep_diverged: bool = False, sink=None, stream_dir: str | None = None, max_batch: int = 256,
                    jpeg_quality: int | None = None, **script_kw):
    """The counterpart of record_sim_episodes.py:68-212 with a scripted teleoperator in the headset's place (av_aloha_amd/scripted.py):
    `num_episodes` episodes of `task_name` ("sim_insert_peg", ...) are run SIDE BY SIDE on the device -- one env each, object poses from the
    task's own reset sampling (global numpy RNG, `seed` seeds it) -- through the Cartesian-action env (sim_env.py:277-312), and come back as
    a list of episode dicts in the layout of record_sim_episodes.py:155-212 (`/observations/{qpos,qvel,all_qpos}`, `/action` = the joint-space
    control with normalised grippers, `/observations/images/<cam>` u8 (T, H, W, 3); T = steps + 1, float32) next to per-episode
    {"max_reward_reached", "success", "rewards", "diverged"}.

    With cameras the episodes are run in batches sized so that one batch's images stay below `image_budget_bytes` of host memory (every
    step's images are written straight into the per-episode arrays: one copy, not three); the object poses are drawn for ALL episodes first,
    in episode order, so the data set does not depend on the batching.  An env whose state diverged during some step (avsim_get_diag, the
    flag the env facades turn into PhysicsError / `truncated`) was put back to its reset state mid-episode: such an episode is dropped, as the
    reference drops an episode whose physics raised (unless keep_diverged; it is flagged either way).  only_success: keep the episodes whose
    LARGEST reward over time is max_reward -- check_dataset_reward.py:52-58's criterion; "success" is that flag, "final_success" says
    whether the episode also ENDS at max_reward.  sink(episode): called for every kept episode as its batch finishes INSTEAD of collecting
    them (a recorder that writes and forgets keeps one batch in memory; the function then returns the episodes' summaries without "data").
    stream_dir: the episodes are written as they are recorded -- every step's images go straight into `<stream_dir>/episode_<i>.hdf5`
    (hdf5min.StreamWriter: a chunk per frame, as save_episode lays the image stacks out), the tables follow at the end, a dropped episode's file
    is removed, the kept ones are numbered consecutively from the files already there.  No image stays in memory, so the batches are not sized by
    the image budget but by `max_batch`: a step of 32 envs costs what a step of 3 costs (one wave each), which made the budgeted batches the
    slow part of a recording with cameras.  The summaries then carry "path" instead of "data".
    jpeg_quality: the images are kept as JPEG streams of that quality: every step's frames are rendered AND encoded on the device
    (sim_env image_streams -> avsim_render_jpeg) and only the streams come to the host, as evaluate_vec's videos do.  The episodes have the
    compressed layout of save_episode(jpeg_quality=...) -- in memory, handed to `sink`, or written to stream_dir (whole files through
    save_episode: an episode's streams are a few tens of MB).  The streams of a whole batch stay in memory until it ends, so the batches are
    sized by `max_batch` and by `image_budget_bytes` with an episode reckoned at 1/16 of its raw frames (rendered frames at quality 90
    take about 1/26): 56 episodes of zed_cam plus one 480 x 640 camera under the default 8 GiB."""
    from . import scripted
    from .env import sample_object_poses
    from .sim_env import make_sim_env, _TASK_OF_SUBSTRING
    task = next(key for sub, key in _TASK_OF_SUBSTRING if sub in task_name)
    n_all = int(num_episodes)
    if seed is not None:
        np.random.seed(seed)
    poses_all = np.stack([sample_object_poses(task) for _ in range(n_all)])           # the draws of n_all sequential env.reset() calls
    cameras = list(cameras)
    b = lambda a, n: np.asarray(a)[None] if n == 1 else np.asarray(a)                 # batch axis for a single env
    episodes = []
    start = 0
    while start < n_all:
        # batch size from the image budget: T is only known once the script exists, so size it with the longest script (600 steps)
        per_ep = _image_bytes_per_step(cameras) * 601
        if jpeg_quality is not None:            # a batch's streams stay in memory until it ends: reckoned at 1/16 of the raw frames
            n = max(1, min(n_all - start, max_batch, int(image_budget_bytes // max(1, per_ep // 16))))
        else:
            n = min(n_all - start, max_batch) if (per_ep == 0 or stream_dir is not None) else max(1, min(n_all - start, int(image_budget_bytes // per_ep)))
        env = make_sim_env(task_name, cameras=cameras, num_envs=n, device=device)
        env.sim.reset(poses_all[start:start + n])
        obs = env.get_obs(images=jpeg_quality is None)
        home = {k: b(obs["poses"][k], n).copy() for k in ("left", "right", "middle")}
        script = scripted.make_script(scripted.SCRIPT_OF_TASK[task], home, b(obs["qpos"], n), **script_kw)
        T = script.steps() + 1
        max_reward = env.sim.max_reward
        fields = {"/observations/qpos": lambda s: s["joints"]["position"], "/observations/qvel": lambda s: s["joints"]["velocity"],
                  "/observations/all_qpos": lambda s: s["qpos"], "/action": lambda s: s["control"]}
        # per-episode arrays, written step by step
        data = [{name: np.empty((T,) + b(f(obs), n).shape[1:], dtype=np.float32) for name, f in fields.items()} for _ in range(n)]
        writers = None
        streams = [{cam: [] for cam in cameras} for _ in range(n)] if jpeg_quality is not None else None
        if streams is not None:
            if stream_dir is not None:
                os.makedirs(stream_dir, exist_ok=True)
        elif stream_dir is not None:
            from . import hdf5min
            os.makedirs(stream_dir, exist_ok=True)
            writers = [hdf5min.StreamWriter(os.path.join(stream_dir, f".recording_{start + k}.part")) for k in range(n)]
        else:
            for k in range(n):
                for cam in obs.get("images", {}):
                    data[k][f"/observations/images/{cam}"] = np.empty((T,) + b(obs["images"][cam], n).shape[1:], dtype=np.uint8)
        rewards = np.zeros((T - 1, n), dtype=np.int32)
        diverged = np.zeros(n, dtype=bool)

        def put(t, o):
            for name, f in fields.items():
                v = b(f(o), n)
                for k in range(n):
                    data[k][name][t] = v[k]
            if streams is not None:             # rendered and encoded on the device: only the streams come to the host
                for cam, ss in env.image_streams(jpeg_quality).items():
                    for k in range(n):
                        streams[k][cam].append(ss[k])
            for cam, img in o.get("images", {}).items():
                img = b(img, n)
                for k in range(n):
                    if writers is not None:
                        writers[k].append(f"/observations/images/{cam}", img[k])
                    else:
                        data[k][f"/observations/images/{cam}"][t] = img[k]
        try:
            put(0, obs)
            for t in range(1, T):
                _, rw, _ = env.sim.step_cartesian(script.action(b(obs["qpos"], n)))
                diverged |= (env.sim.diag()[:, 3] & 1).astype(bool)
                rewards[t - 1] = rw
                obs = env.get_obs(images=jpeg_quality is None)
                put(t, obs)
        except BaseException:
            for w in writers or []:
                w.abort()                       # (no half-written episode files behind a failed recording)
            raise
        finally:
            env.close()
        for k in range(n):
            reached = int(rewards[:, k].max())
            ok = reached == max_reward
            if (only_success and not ok) or (diverged[k] and not keep_diverged):
                if writers is not None:
                    writers[k].abort()
                continue
            if streams is not None:
                data[k].update(pack_streams(streams[k]))
                streams[k] = None
            if stream_dir is not None:
                i = 0
                while os.path.exists(os.path.join(stream_dir, f"episode_{i}.hdf5")):
                    i += 1
                path = os.path.join(stream_dir, f"episode_{i}.hdf5")
                if writers is not None:
                    writers[k].finish(data[k], attrs={"sim": np.bool_(True)})
                    os.replace(writers[k].path, path)
                else:
                    save_episode(data[k], stream_dir, i, jpeg_quality=jpeg_quality)
                    data[k] = None
                episodes.append({"path": path, "success": bool(ok), "final_success": bool(rewards[-1, k] == max_reward), "max_reward_reached": reached,
                                 "rewards": rewards[:, k].copy(), "max_reward": int(max_reward), "diverged": bool(diverged[k]), "episode_index": start + k, "steps": T})
                continue
            ep = {"data": data[k], "success": bool(ok), "final_success": bool(rewards[-1, k] == max_reward), "max_reward_reached": reached,
                             "rewards": rewards[:, k].copy(), "max_reward": int(max_reward), "diverged": bool(diverged[k]), "episode_index": start + k}
            if sink is not None:
                sink(ep)
                ep = {k2: v for k2, v in ep.items() if k2 != "data"}
                data[k] = None
            episodes.append(ep)
        start += n
    return episodes


def check_dataset_reward(gym_id: str, episodes: list, device: int = 0):
    """gym_guided_vision/scripts/check_dataset_reward.py:15-63 for a list of episode dicts (or loaded files): the gym env of the task is put
    into the episode's first recorded state (`set_qpos(all_qpos[0])`) and steps the recorded `/action` sequence OPEN LOOP through `step_action`
    -- on the gym assets' model, whose peg / needle contacts are stiffer than those of the data-collection assets the episode was recorded on
    (task_insert_peg.xml:7 "HACK: modified solref different from data collection") --, `get_reward()` after every step; an episode passes when
    its largest reward is `max_reward`.  All episodes are replayed side by side in one batched env.  -> (passed bool [n], rewards int [T, n])
    The images are never read, so an episode of a compressed file (save_episode(jpeg_quality=...)) is checked as it is."""
    from .env import make
    n = len(episodes)
    q0 = np.stack([np.asarray(e["/observations/all_qpos"][0], dtype=np.float64) for e in episodes])
    acts = np.stack([np.asarray(e["/action"], dtype=np.float32) for e in episodes], axis=1)          # [T, n, 21]
    env = make(gym_id, cameras=[], num_envs=n, device=device)
    env.reset()
    env.set_qpos(q0)
    rewards = np.zeros((acts.shape[0], n), dtype=np.int32)
    for t in range(acts.shape[0]):
        env.step_action(acts[t][:, :env.num_joints])
        rewards[t] = np.asarray(env.get_reward()).reshape(n)
    ok = rewards.max(axis=0) == env.max_reward
    env.close()
    return ok, rewards


def pack_streams(streams: dict) -> dict:
    """{camera: [JPEG streams of the T frames]} -> the image part of a compressed episode, the layout of the ALOHA data sets:
    `/observations/images/<cam>` u8 [T, max_len] (every stream zero-padded to the longest of the episode) and `/compress_len` int32
    [ncam, T] (rows in sorted camera-name order)."""
    cams = sorted(streams)
    T = len(streams[cams[0]]) if cams else 0
    assert all(len(streams[c]) == T for c in cams), "every camera has a stream per frame"
    width = max((len(x) for c in cams for x in streams[c]), default=0)
    out = {"/compress_len": np.array([[len(x) for x in streams[c]] for c in cams], dtype=np.int32).reshape(len(cams), T)}
    for c in cams:
        table = np.zeros((T, width), dtype=np.uint8)
        for t, x in enumerate(streams[c]):
            table[t, :len(x)] = np.frombuffer(x, np.uint8)
        out[f"/observations/images/{c}"] = table
    return out


def compress_episode(data: dict, jpeg_quality: int, encoder=None) -> dict:
    """An episode with u8 (T, H, W, 3) image stacks -> the same episode with the stacks as JPEG streams (pack_streams).  encoder: a
    BatchedSim to encode on the device (encode_jpeg); None: av_aloha_amd.jpeg.encode_reference on the host, the same bytes, slowly."""
    from . import jpeg
    images = {k: v for k, v in data.items() if "/images/" in k}
    out = {k: v for k, v in data.items() if k not in images}
    enc = (lambda v: encoder.encode_jpeg(np.ascontiguousarray(v), jpeg_quality)) if encoder is not None else \
        (lambda v: [jpeg.encode_reference(f, jpeg_quality) for f in np.asarray(v)])
    out.update(pack_streams({k.rsplit("/", 1)[1]: enc(v) for k, v in images.items()}))
    return out


def save_episode(data: dict, dataset_dir: str, episode_idx: int, use_h5py: bool | None = None, jpeg_quality: int | None = None, encoder=None) -> str:
    """episode_<idx>.hdf5 with the reference's layout (record_sim_episodes.py:186-206): through h5py when it is importable
    (use_h5py None / True), else through av_aloha_amd.hdf5min.
    jpeg_quality: the compressed layout the reference left commented out (record_sim_episodes.py:202-203) and the ALOHA data sets use:
    `/observations/images/<cam>` u8 [T, max_len] JPEG streams of this project's encoder, zero-padded; `/compress_len` int32 [ncam, T],
    rows in sorted camera-name order; attributes compress = True and jpeg_quality.  `data` holds either the raw u8 (T, H, W, 3) stacks,
    which are encoded here (compress_episode; encoder: a BatchedSim to do it on the device), or streams that are packed already
    (`/compress_len` present: record_scripted's).  load_episode(decode=...) gives the stacks back."""
    os.makedirs(dataset_dir, exist_ok=True)
    base = os.path.join(dataset_dir, f"episode_{episode_idx}")
    attrs = {"sim": np.bool_(True)}
    if jpeg_quality is not None:
        if "/compress_len" not in data:
            data = compress_episode(data, jpeg_quality, encoder)
        attrs.update({"compress": np.bool_(True), "jpeg_quality": np.int32(jpeg_quality)})
    h5py = None
    if use_h5py is not False:
        try:
            import h5py
        except ImportError:
            if use_h5py:
                raise
    if h5py is None:
        from . import hdf5min
        chunks = {k: (1, *v.shape[1:]) for k, v in data.items() if "/images/" in k and jpeg_quality is None}
        hdf5min.write(base + ".hdf5", data, attrs=attrs, chunks=chunks)
        return base + ".hdf5"
    with h5py.File(base + ".hdf5", "w", rdcc_nbytes=1024 ** 2 * 2) as root:
        for k, v in attrs.items():
            root.attrs[k] = v
        for name, array in data.items():
            chunks = (1, *array.shape[1:]) if "/images/" in name and jpeg_quality is None else None
            root.create_dataset(name, data=array, chunks=chunks)
    return base + ".hdf5"


def episode_streams(data: dict) -> dict:
    """{camera: [T JPEG streams]} of a loaded compressed episode (`/compress_len` and the padded tables)."""
    cams = sorted(k.rsplit("/", 1)[1] for k in data if "/images/" in k)
    ln = np.asarray(data["/compress_len"])
    assert ln.shape[0] == len(cams), "/compress_len has a row per camera"
    return {c: [np.asarray(data[f"/observations/images/{c}"][t, :ln[i, t]]).tobytes() for t in range(ln.shape[1])] for i, c in enumerate(cams)}


def load_episode(path: str, decode=None) -> dict:
    """The data sets of an episode file.  decode None: what the file holds -- of a compressed file (save_episode(jpeg_quality=...)) the
    padded stream tables and `/compress_len`.  decode "host": a compressed file's images as u8 (T, H, W, 3) stacks through
    av_aloha_amd.jpeg.decode_reference (slow: a Python loop per coefficient); a BatchedSim: the same stacks through the device
    (decode_jpeg).  `/compress_len` is dropped then; a raw file is returned as it is either way."""
    if path.endswith(".npz"):
        with np.load(path) as z:
            out = {k: z[k] for k in z.files if k != "sim"}
    else:
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is None:
            from . import hdf5min
            out = hdf5min.read(path)[0]
        else:
            out = {}
            with h5py.File(path, "r") as root:
                root.visititems(lambda n, o: out.__setitem__("/" + n, o[()]) if hasattr(o, "shape") else None)
    if decode is None or "/compress_len" not in out:
        return out
    from . import jpeg
    streams = episode_streams(out)
    del out["/compress_len"]
    for cam, ss in streams.items():
        if isinstance(decode, str):
            if decode != "host":
                raise ValueError(f"load_episode: decode {decode!r} (None, 'host' or a BatchedSim)")
            out[f"/observations/images/{cam}"] = np.stack([jpeg.decode_reference(x) for x in ss])
        else:
            out[f"/observations/images/{cam}"] = decode.decode_jpeg(ss)
    return out


class _HostComposer:
    """visualize_*'s steps through the specifications (compose.py, jpeg.py): for the CPU tests and for small files."""

    def __init__(self):
        self.bytes_to_device = self.bytes_from_device = 0

    def images(self, frames=None, streams=None):
        from . import jpeg
        return np.ascontiguousarray(frames) if streams is None else np.stack([jpeg.decode_reference(x) for x in streams])

    def compose(self, src, places, canvas, canvas_hw, n):
        from .compose import compose_reference
        canvas = np.zeros((n, canvas_hw[0], canvas_hw[1], 3), np.uint8) if canvas is None else canvas
        return compose_reference(canvas, src, places)

    def label(self, canvas, where, prefix, values):
        from .compose import label_reference
        return label_reference(canvas, where, prefix, values, 0xFFFFFF)

    def encode(self, canvas, quality):
        from . import jpeg
        return [jpeg.encode_reference(f, quality) for f in canvas]

    def close(self):
        pass


class _DeviceComposer:
    """The same steps on the device (images.DeviceImages: avsim_jpeg_decode, avsim_compose, avsim_compose_label, avsim_jpeg_encode):
    streams or raw frames go in, streams come out, and no decoded or composed pixel leaves the device."""

    def __init__(self, device):
        from .images import DeviceImages
        self.img = DeviceImages(int(device))
        self.torch = self.img.torch
        self.bytes_to_device = self.bytes_from_device = 0
        self._status = []          # of the decode calls since the last encode, read when that waits for the stream anyway

    def _up(self, a):
        self.bytes_to_device += a.nbytes
        return self.torch.from_numpy(a).to(self.img.device)

    def images(self, frames=None, streams=None):
        from . import jpeg
        if streams is None:
            return self._up(np.ascontiguousarray(frames))
        H, W = jpeg.stream_size(streams[0])
        stride = max(len(x) for x in streams)
        buf, ln = np.zeros((len(streams), stride), np.uint8), np.array([len(x) for x in streams], np.int32)
        for i, x in enumerate(streams):
            buf[i, :len(x)] = np.frombuffer(x, np.uint8)
        out, status = self.img.decode_jpeg(self._up(buf), self._up(ln), height=H, width=W, fmt="gym")
        self._status.append(status)
        return out

    def compose(self, src, places, canvas, canvas_hw, n):
        return self.img.compose(src, places, out=canvas, canvas_hw=canvas_hw, nout=n, clear=0 if canvas is None else None)

    def label(self, canvas, where, prefix, values):
        v = None if values is None else self._up(np.ascontiguousarray(values, dtype=np.int64))
        return self.img.compose_label(canvas, where, prefix, v, 0xFFFFFF)

    def encode(self, canvas, quality):
        out, ln = self.img.encode_images(canvas, quality)
        n = ln.cpu().numpy()                                       # (waits for the stream)
        if int(n.max()) > out.shape[1]:                            # some stream did not fit: its length says what it needs
            out = self.torch.empty((len(n), int(n.max())), dtype=self.torch.uint8, device=self.img.device)
            out, ln = self.img.encode_images(canvas, quality, out=out)
            n = ln.cpu().numpy()
        status, self._status = self._status, []
        if any(bool(st.any().item()) for st in status):
            raise ValueError("visualize: an episode's JPEG stream is not one of this project's encoder")
        data = out[:, :int(n.max())].cpu().numpy()
        self.bytes_from_device += data.nbytes + n.nbytes
        return [data[i, :n[i]].tobytes() for i in range(len(n))]

    def close(self):
        self.img.close()


def _visualize(episodes, video_path, cameras, stride, prefix, numbered, quality, fps, device, chunk_bytes):
    """episodes: an iterable of (number, loaded episode dict).  -> a summary dict."""
    import time
    from . import jpeg
    from .compose import layout_row
    from .mjpeg import AviWriter
    if int(stride) < 1:
        raise ValueError(f"visualize: stride {stride}")
    comp = _HostComposer() if device == "host" else _DeviceComposer(device)
    writer, frames, t_start = None, 0, time.time()
    try:
        for number, data in episodes:
            compressed = "/compress_len" in data
            have = sorted(k.rsplit("/", 1)[1] for k in data if k.startswith("/observations/images/"))
            cams = have if cameras is None else sorted(cameras)
            if not cams or any(c not in have for c in cams):
                raise ValueError(f"visualize: cameras {cams} of an episode that holds {have}")
            streams = episode_streams(data) if compressed else None
            sizes = [jpeg.stream_size(streams[c][0]) if compressed else tuple(data[f"/observations/images/{c}"].shape[1:3]) for c in cams]
            rows, CH, CW = layout_row(sizes)
            if writer is None:
                os.makedirs(os.path.dirname(os.path.abspath(video_path)), exist_ok=True)
                writer = AviWriter(video_path, CW, CH, fps=fps)
            elif (writer.height, writer.width) != (CH, CW):
                raise ValueError(f"visualize: episode {number} gives {CH} x {CW} frames, the video has {writer.height} x {writer.width}")
            T = len(streams[cams[0]]) if compressed else data[f"/observations/images/{cams[0]}"].shape[0]
            ts = list(range(0, T, int(stride)))
            per_frame = sum(h * w * 3 for h, w in sizes) + 2 * CH * CW * 3
            chunk = max(1, int(chunk_bytes) // per_frame)
            for c0 in range(0, len(ts), chunk):
                tt = ts[c0:c0 + chunk]
                n, canvas = len(tt), None
                for cam, (x0, y0, w, h) in zip(cams, rows):      # one call per camera onto the same canvas, cleared by the first
                    src = comp.images(streams=[streams[cam][t] for t in tt]) if compressed else comp.images(frames=data[f"/observations/images/{cam}"][tt])
                    canvas = comp.compose(src, [(i, i, x0, y0, w, h) for i in range(n)], canvas, (CH, CW), n)
                if prefix is not None:
                    canvas = comp.label(canvas, [(i, 10, 10, 3) for i in range(n)], prefix, [number] * n if numbered else None)
                for x in comp.encode(canvas, quality):
                    writer.add(x)
                frames += n
        if writer is None:
            raise ValueError("visualize: no episodes")
        writer.close()
    except BaseException:
        if writer is not None:
            writer.abort()
        raise
    finally:
        comp.close()
    return {"video_path": video_path, "frames": frames, "seconds": time.time() - t_start, "bytes_to_device": comp.bytes_to_device,
            "bytes_from_device": comp.bytes_from_device}


def visualize_episode(path_or_data, video_path, cameras=None, stride=1, label=None, quality=90, fps=None, device=0, chunk_bytes=256 << 20):
    """gym_guided_vision/scripts/visualize_episodes.py:47-98 `save_videos`: the cameras of one episode (a path, or a loaded dict; sorted by
    name, or the given ones) side by side at the smallest camera's height (compose.layout_row: new_w = int(min_h * w / h)), every stride-th
    frame, as ONE Motion-JPEG AVI (mjpeg.AviWriter; fps defaults to 50).  label: a text of at most 15 characters written at (10, 10).
    A compressed file's streams are decoded on the device, a raw file's frames uploaded as u8, in chunks of about chunk_bytes of device
    memory; each chunk is composed with one avsim_compose call per camera and encoded there, and only the streams come back.
    device="host": the same steps through compose_reference and jpeg.encode_reference -- the same bytes, slowly (tests, small files).
    The resampling is Pillow's antialiased bilinear, not cv2.resize's; the joint plots of the reference script are not made.
    -> {"video_path", "frames", "seconds", "bytes_to_device", "bytes_from_device"}."""
    data = load_episode(path_or_data) if isinstance(path_or_data, str) else path_or_data
    return _visualize([(0, data)], video_path, cameras, stride, label, False, quality, 50 if fps is None else fps, device, chunk_bytes)


def visualize_dataset(paths, video_path, stride=20, cameras=None, label="EPISODE ", quality=90, fps=None, device=0, chunk_bytes=256 << 20):
    """gym_guided_vision/scripts/visualize_all_episodes.py:30-121: every stride-th frame of every episode file in ONE video, each frame
    labelled `EPISODE <i>` at (10, 10) (label: the prefix; None: no label).  paths: the files (or a glob pattern); they are sorted by episode
    number and must be numbered 0, 1, 2, ... without gaps (:53-61), else ValueError.  fps defaults to int(1 / SIM_DT / 10), the reference's.
    The rest as visualize_episode."""
    import glob
    import re
    from .constants import SIM_DT
    paths = sorted(glob.glob(paths)) if isinstance(paths, str) else list(paths)
    if not paths:
        raise ValueError("visualize_dataset: no episode files")
    number = {}
    for p in paths:
        m = re.fullmatch(r"episode_(\d+)\.hdf5", os.path.basename(p))
        if m is None:
            raise ValueError(f"visualize_dataset: {p} is not an episode_<i>.hdf5 file")
        number[p] = int(m.group(1))
    paths = sorted(paths, key=number.get)
    for i, p in enumerate(paths):
        if number[p] != i:
            raise ValueError(f"visualize_dataset: episode_{i}.hdf5 is missing (the files must be numbered without gaps)")
    return _visualize(((number[p], load_episode(p)) for p in paths), video_path, cameras, stride, label, True, quality,
                      int(1 / SIM_DT / 10) if fps is None else fps, device, chunk_bytes)


def replay_episode(env, data: dict):
    """Drives `env` (gym flavour, av_aloha_amd.env) through the recorded full states; returns the observations and rewards."""
    env.reset()
    obs, rewards = [], []
    na = 14 if env.num_arms == 2 else 21
    for q in data["/observations/all_qpos"]:
        env.set_qpos(np.asarray(q, dtype=np.float64))
        obs.append(env.get_obs()["agent_pos"][..., :na])
        rewards.append(env.get_reward())
    return np.stack(obs), np.asarray(rewards)


def rerender_episode(data, env_id: str, save_path: str | None = None, device: int = 0, frames_per_batch: int = 128, env=None, use_h5py: bool | None = None):
    """gym_guided_vision/scripts/replay_sim_episode.py:47-89 `replay_episode`: `data` is an episode (a path or a loaded dict with
    `/observations/{qpos,qvel,all_qpos}` and `/action`); `env_id` names the gym env whose camera configuration the new data set is for
    (`gym_guided_vision/<Task>-{2,3}Arms-v0`: 6 cameras for 3 arms, 4 for 2, 480 x 640, __init__.py:6-19).  Every recorded full state
    `all_qpos[t]` is put back (`set_qpos`, env.py:251-253) and the env's cameras are rendered (`get_obs()["pixels"]`, env.py:180-188); the
    result holds `/observations/qpos`, `/observations/qvel`, `/action` -- the first 14 columns for a 2-arm env, all 21 otherwise (:62-73) --
    and `/observations/images/<cam>` u8 (T, H, W, 3) per camera; `all_qpos` is not carried over (the reference's data_dict does not have it).
    The frames are independent, so they are T envs of one batched handle, `frames_per_batch` at a time (one set_qpos + one render call each).
    save_path: also written there in the reference's layout (replay_sim_episode.py:11-44).  env: a batched gym env of `env_id` with
    num_envs == frames_per_batch to reuse (rerender_dataset passes one).  The episode's own images are never read -- the frames are drawn
    anew --, so a compressed file (save_episode(jpeg_quality=...)) is rendered again as it is."""
    from .env import ENVS, make
    if isinstance(data, str):
        data = load_episode(data)
    spec = ENVS[env_id]
    all_qpos = np.asarray(data["/observations/all_qpos"], dtype=np.float64)
    T = all_qpos.shape[0]
    na = 14 if spec["num_arms"] == 2 else 21
    out = {"/observations/qpos": np.ascontiguousarray(np.asarray(data["/observations/qpos"])[:, :na]),
           "/observations/qvel": np.ascontiguousarray(np.asarray(data["/observations/qvel"])[:, :na]),
           "/action": np.ascontiguousarray(np.asarray(data["/action"])[:, :na])}
    own = env is None
    B = max(1, min(int(frames_per_batch), T)) if own else env.num_envs
    if own:
        env = make(env_id, num_envs=B, device=device)
    assert env.num_arms == spec["num_arms"] and list(env.cameras) == list(spec["cameras"]), "env does not have the camera configuration of env_id"
    H, W = env.observation_height, env.observation_width
    for cam in env.cameras:
        out[f"/observations/images/{cam}"] = np.empty((T, H, W, 3), dtype=np.uint8)
    nq = env.sim.nq
    assert all_qpos.shape[1] == nq, f"the episode's all_qpos has {all_qpos.shape[1]} columns, the model of {env_id} {nq}"
    for t0 in range(0, T, B):
        q = all_qpos[t0:t0 + B]
        n = q.shape[0]
        if n < B:                                   # the last chunk: the spare envs repeat its last frame
            q = np.concatenate([q, np.repeat(q[-1:], B - n, 0)])
        env.sim.set_qpos(q)
        if n == B:      # a full chunk: every camera's frames straight from the device into their place in the episode's array
            for cam in env.cameras:
                env.sim.render_rgb([cam], H, W, cam_major=True, out=out[f"/observations/images/{cam}"][t0:t0 + B])
        else:
            img = env.sim.render_rgb(env.cameras, H, W, cam_major=True)   # [ncam, B, H, W, 3]: a camera's frames are one contiguous block
            for ci, cam in enumerate(env.cameras):
                out[f"/observations/images/{cam}"][t0:t0 + n] = img[ci, :n]
    if own:
        env.close()
    if save_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
        d, f = os.path.split(os.path.abspath(save_path))
        assert f.startswith("episode_") and f.endswith(".hdf5"), "save_path is <dir>/episode_<i>.hdf5 (replay_sim_episode.py:104-107)"
        save_episode(out, d, int(f[len("episode_"):-len(".hdf5")]), use_h5py=use_h5py)
    return out


def rerender_pointclouds(data, env_id: str, cameras, height: int, width: int, bounds, points: int, frames_per_batch: int = 128, max_depth=None, device: int = 0, sim=None):
    """The point clouds of a recorded episode, as an evaluation with VecEnv(pointcloud=...) will see them: (xyz float32 [T, P, 3], count int32
    [T, 2]).  Works as rerender_episode does -- every recorded full state `all_qpos[t]` is put back (`set_qpos`), T frames as T envs of one
    batched handle, `frames_per_batch` at a time -- and calls BatchedSim.point_cloud (depth render + avsim_point_cloud) on each batch.
    sim: a BatchedSim of env_id's task and arms to reuse (its num_envs is the batch then)."""
    from .env import ENVS
    from .sim import BatchedSim
    from .vec_env import _TASK_OF_CLASS
    if isinstance(data, str):
        data = load_episode(data)
    spec = ENVS[env_id]
    all_qpos = np.asarray(data["/observations/all_qpos"], dtype=np.float64)
    T = all_qpos.shape[0]
    own = sim is None
    B = max(1, min(int(frames_per_batch), T)) if own else sim.N
    if own:
        sim = BatchedSim(_TASK_OF_CLASS[spec["env"]], spec["num_arms"], B, device=device)
    assert all_qpos.shape[1] == sim.nq, f"the episode's all_qpos has {all_qpos.shape[1]} columns, the model of {env_id} {sim.nq}"
    xyz, count = np.empty((T, int(points), 3), dtype=np.float32), np.empty((T, 2), dtype=np.int32)
    for t0 in range(0, T, B):
        q = all_qpos[t0:t0 + B]
        n = q.shape[0]
        if n < B:                                   # the last chunk: the spare envs repeat its last frame
            q = np.concatenate([q, np.repeat(q[-1:], B - n, 0)])
        sim.set_qpos(q)
        x, _, c = sim.point_cloud(cameras, height, width, bounds, points, max_depth=max_depth)
        xyz[t0:t0 + n], count[t0:t0 + n] = x[:n], c[:n]
    if own:
        sim.h.close()
    return xyz, count


def parse_pointcloud_option(text: str) -> dict:
    """"cams:h:w:P:xlo,ylo,zlo,xhi,yhi,zhi" (cams: comma-separated camera names) as rerender_pointclouds' keyword arguments."""
    parts = text.split(":")
    if len(parts) != 5:
        raise ValueError("--pointcloud cams:h:w:P:xlo,ylo,zlo,xhi,yhi,zhi")
    b = [float(v) for v in parts[4].split(",")]
    if len(b) != 6:
        raise ValueError("--pointcloud: six bounds xlo,ylo,zlo,xhi,yhi,zhi")
    return {"cameras": [c for c in parts[0].split(",") if c], "height": int(parts[1]), "width": int(parts[2]), "points": int(parts[3]), "bounds": b}


def rerender_dataset(dataset_dir: str, env_id: str, episode_idx: int | None = None, device: int = 0, frames_per_batch: int = 128, pointcloud: dict | None = None):
    """replay_sim_episode.py:92-113 `main`: every `episode_*.hdf5` of `dataset_dir` (or the one with `episode_idx`) re-rendered for
    `env_id` into `<dataset_dir>/<EnvName>/episode_<i>.hdf5` (EnvName = the id without its namespace).  Returns the written paths and
    the frames per second over the whole run.  pointcloud: rerender_pointclouds' cameras / height / width / bounds / points -- the clouds are
    written as `/observations/pointcloud` (and `/observations/pointcloud_count`) next to the images."""
    import glob
    import time
    from .env import make
    pat = "episode_*.hdf5" if episode_idx is None else f"episode_{episode_idx}.hdf5"
    paths = sorted(glob.glob(os.path.join(dataset_dir, pat)))
    env = make(env_id, num_envs=frames_per_batch, device=device) if paths else None
    written, frames, t0 = [], 0, time.time()
    for p in paths:
        save_path = os.path.join(dataset_dir, env_id.split("/")[-1], os.path.basename(p))
        if pointcloud is None:
            out = rerender_episode(p, env_id, save_path, env=env)
        else:           # + /observations/pointcloud [T, P, 3] and /observations/pointcloud_count [T, 2] next to the images
            out = rerender_episode(p, env_id, None, env=env)
            out["/observations/pointcloud"], out["/observations/pointcloud_count"] = rerender_pointclouds(p, env_id, frames_per_batch=frames_per_batch, device=device, sim=env.sim, **pointcloud)
            d, f = os.path.split(os.path.abspath(save_path))
            save_episode(out, d, int(f[len("episode_"):-len(".hdf5")]))
        frames += out["/action"].shape[0]
        written.append(save_path)
    if env is not None:
        env.close()
    dt = time.time() - t0
    return written, (frames / dt if dt > 0 else 0.0)
