"""A data set of compressed episodes (harness.save_episode(jpeg_quality=...), tools/record_scripted_episodes.py --jpeg_quality) whose
batches are decoded on the device: the JPEG streams wait in pinned host memory, a batch's streams cross to the device -- some 26 times
fewer bytes than the frames they hold -- and one avsim_jpeg_decode call per camera turns them into the float32 [B, 3, H, W]
observations a policy reads in VecEnv, on torch's current stream."""
import numpy as np

from . import _ffi, jpeg
from .harness import load_episode


class CompressedDataset:
    """paths: episode files of one task and one image size per camera; cameras: the `/observations/images/<cam>` to serve.  The tables and
    the streams are read once (they are small).  len(ds) counts frames, in the order of `paths`; ds.batch(indices) -> dict of tensors on
    `device`: "observation.images.<cam>" float32 [B, 3, H, W] in [0, 1] ((float)u8 / 255 of jpeg.decode_reference's pixels),
    "observation.state" float32 [B, 21 | 14], "action", "episode_index" and "frame_index" int64 [B]; ds.batches(batch_size, seed) walks a
    shuffled epoch.  batch() does not wait for the device.  check: a stream the decoder flags (not this encoder's) raises jpeg.JpegError -- from
    the NEXT batch() call or from close(), when its status is read without holding the decode up; that batch's image is unspecified."""

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
        torch.zeros(1, device=self.device)           # torch's runtime comes up first (vec_env.py)
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
        import os
        from .constants import MODEL_DIR             # the smallest handle the library offers: the decoder needs none of the model
        with open(os.path.join(MODEL_DIR, "insert_peg_3arms.avm"), "rb") as f:
            self.h = _ffi.Handle(f.read(), 2, self.device.index or 0, _ffi.AVSIM_IO_DEVICE)
        self._stage, self._pending = {}, []

    def __len__(self):
        return self.n

    def batch(self, indices):
        torch = self.torch
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if len(idx) == 0 or idx.min() < 0 or idx.max() >= self.n:
            raise IndexError(f"batch indices outside [0, {self.n})")
        B = len(idx)
        t_idx = torch.from_numpy(idx).to(self.device, non_blocking=True)
        out = {"observation.state": self.state[t_idx], "action": self.action[t_idx], "episode_index": self.episode_index[t_idx],
               "frame_index": self.frame_index[t_idx]}
        self.h.check(self.h.L.avsim_set_stream(self.h.h, torch.cuda.current_stream(self.device).cuda_stream))
        self._check_pending()
        for c in self.cameras:
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
            img = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
            status = torch.empty(B, dtype=torch.int32, device=self.device)
            self.h.check(self.h.L.avsim_jpeg_decode(self.h.h, d_rows.data_ptr(), self.stride[c], d_len.data_ptr(), None, B, H, W, 1,
                                                    1 if self.upsample == "triangle" else 0, img.data_ptr(), status.data_ptr()))
            if self.check:
                self._pending.append((status, idx, c))
            out[f"observation.images.{c}"] = img
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
        if getattr(self, "h", None) is not None:
            try:
                self._check_pending()
            finally:
                self.h.close()
                self.h = None
