"""A data set of compressed episodes (harness.save_episode(jpeg_quality=...), tools/record_scripted_episodes.py --jpeg_quality) whose
batches are decoded on the device: the JPEG streams wait in pinned host memory, a batch's streams cross to the device -- some 26 times
fewer bytes than the frames they hold -- and one avsim_jpeg_decode call per camera turns them into the float32 [B, 3, H, W]
observations a policy reads in VecEnv, on torch's current stream."""
import json

import numpy as np

from . import imgaug, imgprep, imgresize, jpeg
from .harness import load_episode
from .images import DeviceImages


class CompressedDataset:
    """paths: episode files of one task and one image size per camera; cameras: the `/observations/images/<cam>` to serve.  The tables and
    the streams are read once (they are small).  len(ds) counts frames, in the order of `paths`; ds.batch(indices) -> dict of tensors on
    `device`: "observation.images.<cam>" float32 [B, 3, H, W] in [0, 1] ((float)u8 / 255 of jpeg.decode_reference's pixels),
    "observation.state" float32 [B, 21 | 14], "action", "episode_index" and "frame_index" int64 [B]; ds.batches(batch_size, seed) walks a
    shuffled epoch.  batch() does not wait for the device.  check: a stream the decoder flags (not this encoder's) raises jpeg.JpegError -- from
    the NEXT batch() call or from close(), when its status is read without holding the decode up; that batch's image is unspecified.
    batch(indices, fmt="gym") hands the images out as the decoder's uint8 [B, H, W, 3] instead (what TrainingBatches and stats() read)."""

    def __init__(self, paths, cameras, device=None, upsample="replicate", check=True):
        import torch
        self.torch = torch
        if upsample not in ("replicate", "triangle"):
            raise ValueError(f"upsample {upsample!r}: 'replicate' or 'triangle'")
        self.upsample, self.check = upsample, check
        self.cameras = list(cameras)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("CompressedDataset decodes on the GPU: device is a cuda device")
        state, action, ep_idx, fr_idx = [], [], [], []
        streams = {c: [] for c in self.cameras}
        for e, path in enumerate(paths):
            d = load_episode(path)
            if "/compress_len" not in d:
                raise ValueError(f"{path}: not a compressed episode (no /compress_len)")
            cams = sorted(k.rsplit("/", 1)[1] for k in d if "/images/" in k)
            T = d["/action"].shape[0]
            for c in self.cameras:
                if c not in cams:
                    raise ValueError(f"{path}: no camera {c!r} (has {cams})")
                ln = d["/compress_len"][cams.index(c)]
                streams[c] += [d[f"/observations/images/{c}"][t, :ln[t]] for t in range(T)]
            state.append(np.asarray(d["/observations/qpos"], np.float32))
            action.append(np.asarray(d["/action"], np.float32))
            ep_idx.append(np.full(T, e, np.int64))
            fr_idx.append(np.arange(T, dtype=np.int64))
        if not state:
            raise ValueError("CompressedDataset: no episodes")
        self.state = torch.from_numpy(np.concatenate(state)).to(self.device)
        self.action = torch.from_numpy(np.concatenate(action)).to(self.device)
        self.episode_index = torch.from_numpy(np.concatenate(ep_idx)).to(self.device)
        self.frame_index = torch.from_numpy(np.concatenate(fr_idx)).to(self.device)
        self.n = int(self.state.shape[0])
        self.ep_len = np.array([len(x) for x in state], dtype=np.int64)      # the episodes' lengths and first global frames (imgprep.chunk_index)
        self.ep_start = np.concatenate([[0], np.cumsum(self.ep_len)[:-1]]).astype(np.int64)
        # per camera: every stream back to back in one pinned buffer, with its offset and length
        self.buf, self.off, self.len, self.size, self.stride = {}, {}, {}, {}, {}
        for c, ss in streams.items():
            ln = np.array([len(x) for x in ss], dtype=np.int64)
            self.off[c], self.len[c] = np.concatenate([[0], np.cumsum(ln)[:-1]]), ln
            flat = torch.empty(int(ln.sum()), dtype=torch.uint8).pin_memory()
            flat.numpy()[:] = np.concatenate(ss)
            self.buf[c] = flat
            self.size[c] = jpeg.stream_size(ss[0].tobytes())
            self.stride[c] = (int(ln.max()) + 255) // 256 * 256
        self.img = DeviceImages(self.device)         # the image calls
        self._stage, self._pending = {}, []

    def __len__(self):
        return self.n

    def batch(self, indices, fmt="lerobot"):
        torch = self.torch
        if fmt not in ("lerobot", "gym"):
            raise ValueError(f"fmt {fmt!r}: 'lerobot' (float32 [B, 3, H, W]) or 'gym' (uint8 [B, H, W, 3])")
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= self.n:
            raise IndexError(f"batch indices outside [0, {self.n})")
        t_idx = torch.from_numpy(idx).to(self.device, non_blocking=True)
        out = {"observation.state": self.state[t_idx], "action": self.action[t_idx], "episode_index": self.episode_index[t_idx],
               "frame_index": self.frame_index[t_idx]}
        self._check_pending()
        for c in self.cameras:
            out[f"observation.images.{c}"] = self._decode(c, idx, fmt)
        return out

    def _decode(self, c, idx, fmt):
        """The frames idx of camera c, decoded on torch's current stream: float32 [B, 3, H, W] (fmt "lerobot") or uint8 [B, H, W, 3] ("gym")."""
        torch = self.torch
        B = len(idx)
        ln = self.len[c][idx]
        if (c, B) not in self._stage:            # pinned rows for a batch of B streams of the camera's longest length, reused by later batches
            self._stage[c, B] = (torch.empty((B, self.stride[c]), dtype=torch.uint8).pin_memory(), torch.empty(B, dtype=torch.int32).pin_memory(),
                                 torch.cuda.Event())
        rows, lens, done = self._stage[c, B]
        done.synchronize()                       # (the copy of the last batch that used these rows)
        src, r = self.buf[c].numpy(), rows.numpy()
        for i, (o, n) in enumerate(zip(self.off[c][idx], ln)):
            r[i, :n] = src[o:o + n]
        lens.numpy()[:] = ln
        d_rows, d_len = rows.to(self.device, non_blocking=True), lens.to(self.device, non_blocking=True)
        done.record()
        H, W = self.size[c]
        img, status = self.img.decode_jpeg(d_rows, d_len, height=H, width=W, upsample=self.upsample, fmt=fmt)
        if self.check:
            self._pending.append((status, idx, c))
        return img

    def stats(self, batch_size=256):
        """The data set's statistics, {key: {"mean", "std", "min", "max"}} as float32 arrays: of every camera ("observation.images.<cam>",
        [3, 1, 1] in units of [0, 1]) over every pixel of every frame -- each frame decoded once as u8 and reduced on the device
        (avsim_image_stats), the integer sums combined exactly (imgprep.combine_stats: no float accumulation, the same result for every
        batch_size) --, and of "observation.state" and "action" per dimension, in float64.  std is the population std."""
        torch = self.torch
        self._check_pending()
        out = {}
        for c in self.cameras:
            H, W = self.size[c]
            sums = torch.empty((self.n, 3, 4), dtype=torch.int64, device=self.device)
            for i0 in range(0, self.n, int(batch_size)):
                idx = np.arange(i0, min(self.n, i0 + int(batch_size)), dtype=np.int64)
                self.img.image_stats(self._decode(c, idx, "gym"), out=sums[i0:i0 + len(idx)])
            out[f"observation.images.{c}"] = imgprep.combine_stats(sums.cpu().numpy().view(np.uint64), H * W)
            self._check_pending()
        for key, t in (("observation.state", self.state), ("action", self.action)):
            x = t.cpu().numpy().astype(np.float64)
            out[key] = {"mean": x.mean(0).astype(np.float32), "std": x.std(0).astype(np.float32), "min": x.min(0).astype(np.float32),
                        "max": x.max(0).astype(np.float32)}
        return out

    def _check_pending(self):
        """The decoder's status of the batches handed out so far (this waits for them: they are the previous batch's, long done)."""
        pending, self._pending = self._pending, []
        for status, idx, c in pending:
            st = status.cpu().numpy()
            if st.any():
                bad = int(np.nonzero(st)[0][0])
                raise jpeg.JpegError(int(st[bad]), f"CompressedDataset: frame {int(idx[bad])} of camera {c!r} is not a {self.size[c][0]} x {self.size[c][1]} stream of this encoder")

    def batches(self, batch_size, seed=0, drop_last=False):
        """One epoch in an order shuffled by `seed`."""
        order = np.random.default_rng(seed).permutation(self.n)
        for i in range(0, self.n, batch_size):
            part = order[i:i + batch_size]
            if drop_last and len(part) < batch_size:
                return
            yield self.batch(part)

    def close(self):
        if getattr(self, "img", None) is not None:
            try:
                self._check_pending()
            finally:
                self.img.close()
                self.img = None


def save_stats(stats, path):
    """CompressedDataset.stats()'s result as JSON (every float32 written as the double that equals it: load_stats gives the same bits)."""
    with open(path, "w") as f:
        json.dump({k: {n: np.asarray(a, dtype=np.float32).astype(np.float64).tolist() for n, a in v.items()} for k, v in stats.items()}, f, indent=1)
    return path


def load_stats(path):
    with open(path) as f:
        return {k: {n: np.asarray(a, dtype=np.float32) for n, a in v.items()} for k, v in json.load(f).items()}


def epoch_plan(n, batch_size, sizes, crop=None, crop_mode="random", seed=0, epoch=0, drop_last=True):
    """The batches of one epoch and their crop boxes, on the host: [(frame indices int64 [B], {camera: int32 [B, 3] rows (x0, y0, 0)})].
    rng = np.random.default_rng([seed, epoch]) draws the epoch's permutation first; then, per batch and per camera in the order of `sizes`
    (a dict camera -> (H, W), in CompressedDataset.cameras' order), with crop = (h, w) and crop_mode "random": y0 and then x0 as
    rng.integers(0, H - h + 1, B) / rng.integers(0, W - w + 1, B); "center": the centred box, nothing drawn.  crop None: the whole image."""
    if crop_mode not in ("random", "center"):
        raise ValueError(f"crop_mode {crop_mode!r}: 'random' or 'center'")
    for c, (H, W) in sizes.items():
        if crop is not None and not (1 <= crop[0] <= H and 1 <= crop[1] <= W):
            raise ValueError(f"crop {tuple(crop)} does not fit camera {c!r} ({H} x {W})")
    rng = np.random.default_rng([int(seed), int(epoch)])
    order = rng.permutation(int(n))
    plan = []
    for i in range(0, int(n), int(batch_size)):
        part = order[i:i + int(batch_size)].astype(np.int64)
        if drop_last and len(part) < batch_size:
            break
        B, boxes = len(part), {}
        for c, (H, W) in sizes.items():
            h, w = (H, W) if crop is None else (int(crop[0]), int(crop[1]))
            box = np.zeros((B, 3), dtype=np.int32)
            if crop_mode == "random":
                box[:, 1] = rng.integers(0, H - h + 1, B)
                box[:, 0] = rng.integers(0, W - w + 1, B)
            else:
                box[:, 0], box[:, 1] = imgprep.center_box((H, W), (h, w))
            boxes[c] = box
        plan.append((part, boxes))
    return plan


class TrainingBatches:
    """The batches a policy of the ACT / diffusion kind trains on, made on the device from a CompressedDataset.  Iterating walks one epoch
    (the first iteration epoch 0, the next epoch 1, ...; epoch_plan says which frames and which crops) and yields dicts of tensors on the
    data set's device:
      "observation.images.<cam>"  float32 [B, 3, h, w]: the frame decoded as u8 and passed through avsim_image_prep -- cropped to
                                  crop = (h, w) (None: the whole image) and every channel looked up in imgprep.normalise_lut(stats) (normalise
                                  False: imgprep.identity_lut(), values in [0, 1]); the bits of imgprep.prep_reference
      "observation.state"         float32 [B, D]: (x - mean) / std in float32
      "action"                    float32 [B, chunk_size, A]: the actions of the frame and of the chunk_size - 1 that follow, clamped to the
                                  episode's last (imgprep.chunk_index, LeRobot's delta_timestamps), normalised alike
      "action_is_pad"             bool [B, chunk_size]: the clamped ones
      "episode_index", "frame_index"  int64 [B]
    augment: None (the default): nothing below applies.  True, or a dict laid over imgaug.DEFAULT_CFG: every camera's images go through
    avsim_image_jitter instead -- LeRobot's image_transforms (brightness, contrast, saturation, hue, sharpness; a random subset per image,
    drawn by imgaug.augment_plan from a stream of its own) applied to the whole decoded frame, then the same crop and normalisation; the bits
    of imgaug.jitter_reference with plan(epoch)'s boxes and augment_plan(epoch)'s parameters.
    A config with an "affine" entry of weight > 0 (imgaug.LEROBOT_CFG) adds torchvision's RandomAffine as a sixth op: the images go through
    avsim_image_augment with imgaug.augment_plan_affine's matrices (one interpolation per config), augment_plan(epoch) carries the matrix as
    a third element, and the bits are imgaug.jitter_affine_reference's.
    n_obs_steps: None (the default): nothing below applies.  K >= 1: for a policy that reads K observations, the image and state entries
    gain an axis -- "observation.images.<cam>" float32 [B, K, 3, h, w], "observation.state" float32 [B, K, D] --, slot K-1 the item's frame
    and slot k the frame K-1-k steps before it, clamped to the episode's first (imgprep.history_index, LeRobot's negative delta_timestamps);
    "observation.state_is_pad" and "observation.images.<cam>_is_pad" bool [B, K] name the clamped ones.  The K frames of an item share its
    crop box and its augmentation parameters (LeRobot transforms a stacked item with one draw); they go through the same avsim_image_prep /
    avsim_image_jitter call as B K outputs.  What obshist.ObsHistory stacks at evaluation.
    resize: None (the default): nothing below applies.  (h, w): for a policy with a fixed input size, the crop box (random or centred, as above;
    crop None: the whole image) becomes the SOURCE REGION of avsim_image_resize and the images are float32 [B, 3, h, w]: the region resized by
    the triangle filter of interpolate(mode="bilinear", antialias=antialias) -- resize_mode "stretch": to the whole output; "pad": with its
    aspect ratio kept, the zero padding on the left and on top (imgresize.resize_with_pad_plan, the VLA policies' resize_with_pad) --, then
    normalised as (v - mean) / std, the padding included; the bits of imgresize.resize_reference.  Without augment that is ONE pass from the
    decoded u8 frames.  With augment it is TWO: avsim_image_jitter / avsim_image_augment as above but without normalisation, into float32
    crops, then avsim_image_resize on those floats (fmt 1, not quantised), which normalises.  With n_obs_steps the K frames of an item share
    the region.  The plans and their draws do not depend on resize.
    stats: CompressedDataset.stats()'s (or load_stats'); a dimension whose std is 0 normalises to nan / inf, as the formula says.
    Like batch(), an iteration step does not wait for the device."""

    def __init__(self, ds, batch_size, chunk_size, stats, crop=None, crop_mode="random", normalise=True, seed=0, drop_last=True, augment=None,
                 n_obs_steps=None, resize=None, resize_mode="stretch", antialias=True):
        torch = ds.torch
        self.n_obs_steps = None if n_obs_steps is None else int(n_obs_steps)
        if self.n_obs_steps is not None and self.n_obs_steps < 1:
            raise ValueError("TrainingBatches: n_obs_steps is at least 1 (or None)")
        self.augment = None if augment is None or augment is False else imgaug.make_cfg(augment)
        self.ds, self.batch_size, self.chunk_size = ds, int(batch_size), int(chunk_size)
        self.crop, self.crop_mode, self.normalise, self.seed, self.drop_last = crop, crop_mode, bool(normalise), int(seed), bool(drop_last)
        if self.batch_size < 1 or self.chunk_size < 1:
            raise ValueError("TrainingBatches: batch_size and chunk_size are at least 1")
        self.sizes = {c: tuple(ds.size[c]) for c in ds.cameras}
        epoch_plan(0, 1, self.sizes, crop, crop_mode)           # (the arguments' checks)
        self.epoch = 0
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))
        self.resize_mode, self.antialias = resize_mode, bool(antialias)
        if self.resize is not None:
            for c, (H, W) in self.sizes.items():           # (the arguments' checks: the mode, the sizes, the ratio cap)
                sb, dst = imgresize.boxes([(0, 0, 0)], (H, W) if crop is None else crop, self.resize, resize_mode)
                imgresize.check_resize((1, H, W), sb, dst, None, self.resize)
        self.lut, self.norm = {}, {}
        for c in ds.cameras:
            st = stats[f"observation.images.{c}"]
            lut = imgprep.normalise_lut(st["mean"], st["std"]) if self.normalise else imgprep.identity_lut()
            self.lut[c] = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32).reshape(1, 3, 256)).to(ds.device)
        self.mean_std = {}
        if (self.augment is not None or self.resize is not None) and self.normalise:
            for c in ds.cameras:
                st = stats[f"observation.images.{c}"]
                self.mean_std[c] = (st["mean"], st["std"])
        for key in ("observation.state", "action"):
            self.norm[key] = (torch.from_numpy(np.asarray(stats[key]["mean"], dtype=np.float32)).to(ds.device),
                              torch.from_numpy(np.asarray(stats[key]["std"], dtype=np.float32)).to(ds.device))

    def __len__(self):
        return self.ds.n // self.batch_size if self.drop_last else -(-self.ds.n // self.batch_size)

    def plan(self, epoch):
        return epoch_plan(self.ds.n, self.batch_size, self.sizes, self.crop, self.crop_mode, self.seed, epoch, self.drop_last)

    def augment_plan(self, epoch):
        """The augmentation of one epoch, batch after batch of plan(epoch): [{camera: (mask int32 [B], factor float32 [B, 5])}], drawn by
        imgaug.augment_plan(B, cfg, seed, epoch, batch, the camera's index in the data set's cameras).  None without augment."""
        if self.augment is None:
            return None
        if imgaug.has_affine(self.augment):      # (mask, factor, matrix float32 [B, 6]) from augment_plan_affine, which needs the camera's size
            return [{c: imgaug.augment_plan_affine(len(part), self.augment, self.seed, epoch, b, k, size=self.sizes[c])[:3] for k, c in enumerate(self.ds.cameras)}
                    for b, (part, _) in enumerate(self.plan(epoch))]
        return [{c: imgaug.augment_plan(len(part), self.augment, self.seed, epoch, b, k) for k, c in enumerate(self.ds.cameras)}
                for b, (part, _) in enumerate(self.plan(epoch))]

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        if self.augment is not None:
            for (part, boxes), aug in zip(self.plan(epoch), self.augment_plan(epoch)):
                yield self.make(part, boxes, aug)
            return
        for part, boxes in self.plan(epoch):
            yield self.make(part, boxes)

    def _norm(self, key, x):
        if not self.normalise:
            return x
        mean, std = self.norm[key]
        return (x - mean) / std

    def make(self, part, boxes, aug=None):
        """The batch of the frames `part` with the crop boxes {camera: int32 [B, 3]}; aug: {camera: (mask, factor)} (augment_plan's), the
        images then go through avsim_image_jitter."""
        ds, torch = self.ds, self.ds.torch
        if self.n_obs_steps is not None:
            return self._make_history(part, boxes, aug)
        raw = ds.batch(part, fmt="gym")
        B = len(part)
        out = {"observation.state": self._norm("observation.state", raw["observation.state"]), "episode_index": raw["episode_index"],
               "frame_index": raw["frame_index"]}
        index, pad = imgprep.chunk_index(ds.ep_start, ds.ep_len, part, self.chunk_size)
        t_index = torch.from_numpy(index).to(ds.device, non_blocking=True)
        out["action"] = self._norm("action", ds.action[t_index])
        out["action_is_pad"] = torch.from_numpy(pad).to(ds.device, non_blocking=True)
        for c in ds.cameras:
            H, W = self.sizes[c]
            h, w = (H, W) if self.crop is None else (int(self.crop[0]), int(self.crop[1]))
            box = np.ascontiguousarray(boxes[c], dtype=np.int32).reshape(B, 3)
            src = raw[f"observation.images.{c}"]
            if self.resize is not None:
                out[f"observation.images.{c}"] = self._resize(src, box, None if aug is None else aug[c], 1, (h, w), self.mean_std.get(c, (None, None)))
            elif aug is not None:
                ms = self.mean_std.get(c, (None, None))
                out[f"observation.images.{c}"] = self._augment(src, box, aug[c], 1, (h, w), ms)
            else:
                out[f"observation.images.{c}"] = ds.img.prep_images(src, self.lut[c], box, (h, w))
        return out

    def _augment(self, src, box, aug, K, out_hw, ms):
        """One camera's images through avsim_image_jitter, or avsim_image_augment when the plan carries matrices; every item's parameters K times."""
        rep = [np.repeat(a, K, axis=0) for a in aug] if K > 1 else list(aug)
        params = imgaug.pack_params(box, rep[0], rep[1])
        if len(rep) == 2:
            return self.ds.img.jitter_images(src, params, out_hw, mean=ms[0], std=ms[1])
        return self.ds.img.augment_images(src, params, rep[2], out_hw, interp=imgaug.interp_of(self.augment), mean=ms[0], std=ms[1])

    def _resize(self, src, box, aug, K, crop_hw, ms):
        """One camera's images through avsim_image_resize, the crop boxes as source regions: from the u8 frames, or, with aug, from the float
        crops the augmentation made without normalising; mean / std are applied here."""
        if aug is not None:
            src = self._augment(src, box, aug, K, crop_hw, (None, None))
            box = np.zeros((len(box), 3), dtype=np.int32)
        sb, dst = imgresize.boxes(box, crop_hw, self.resize, self.resize_mode)
        return self.ds.img.resize_images(src, sb, dst, self.resize, self.antialias, mean=ms[0], std=ms[1])

    def _make_history(self, part, boxes, aug):
        """make() with n_obs_steps = K: the B K frames of history_index through the same calls, every item's box and parameters K times."""
        ds, torch = self.ds, self.ds.torch
        B, K = len(part), self.n_obs_steps
        hidx, hpad = imgprep.history_index(ds.ep_start, ds.ep_len, part, K)
        raw = ds.batch(hidx.reshape(-1), fmt="gym")
        t_pad = torch.from_numpy(hpad).to(ds.device, non_blocking=True)
        out = {"observation.state": self._norm("observation.state", raw["observation.state"]).reshape(B, K, -1), "observation.state_is_pad": t_pad,
               "episode_index": raw["episode_index"].reshape(B, K)[:, K - 1], "frame_index": raw["frame_index"].reshape(B, K)[:, K - 1]}
        index, pad = imgprep.chunk_index(ds.ep_start, ds.ep_len, part, self.chunk_size)
        t_index = torch.from_numpy(index).to(ds.device, non_blocking=True)
        out["action"] = self._norm("action", ds.action[t_index])
        out["action_is_pad"] = torch.from_numpy(pad).to(ds.device, non_blocking=True)
        for c in ds.cameras:
            H, W = self.sizes[c]
            h, w = (H, W) if self.crop is None else (int(self.crop[0]), int(self.crop[1]))
            box = np.repeat(np.ascontiguousarray(boxes[c], dtype=np.int32).reshape(B, 3), K, axis=0)
            src = raw[f"observation.images.{c}"]
            if self.resize is not None:
                img = self._resize(src, box, None if aug is None else aug[c], K, (h, w), self.mean_std.get(c, (None, None)))
            elif aug is not None:
                ms = self.mean_std.get(c, (None, None))
                img = self._augment(src, box, aug[c], K, (h, w), ms)
            else:
                img = ds.img.prep_images(src, self.lut[c], box, (h, w))
            out[f"observation.images.{c}"] = img.reshape(B, K, 3, *img.shape[2:])
            out[f"observation.images.{c}_is_pad"] = t_pad
        return out
