"""What the device JPEG decoder (avsim_jpeg_decode) costs and what it saves.  Writes profiles/jpeg_decode_<tag>.json.

    python tools/bench_jpeg_decode.py --frames 256,1024 --tag r09 [--record 32]
    rocprofv3 --kernel-trace --stats -d trace -- python tools/bench_jpeg_decode.py --decode-only 256     # the three kernels' shares, in a run of its own

* decode: HIP events around avsim_jpeg_decode of n rendered 480 x 640 frames (SlotInsertion, zed_cam_left) encoded at quality 90, to
  float32 CHW with either upsampling mode and to u8 HWC; and, with the library's option "jpeg_decode_events", HIP events between the
  call's three kernels (index, entropy, reconstruct).
* frames into the GPU, the comparison a trainer cares about: pinned streams -> H2D -> decode to float32 CHW, against pinned raw u8 frames
  -> H2D -> permute().float() / 255 in torch.  Same frames; the two sides alternate in one process; medians over the rounds.
* host decode for scale: Pillow on 16 processes over the same streams.
* --record N: harness.record_scripted of N SlotInsertion episodes with two cameras into a stream_dir, compressed (jpeg_quality 90) against
  raw (every frame straight into its episode file): wall time and the files' bytes.  The files go to a temporary directory (--record-dir
  names its parent) and are removed.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, QUALITY = 480, 640, 90


def pillow_decode(stream):
    from PIL import Image
    import numpy as np
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB")).shape[0]


def streams_of(n):
    """(env, frames u8 [n, H, W, 3], streams u8 [n, stride], lengths int32 [n]) on the device."""
    import torch
    from bench_jpeg import encode_call, rendered_frames
    env, frames = rendered_frames(n)
    out = torch.empty((n, 128 << 10), dtype=torch.uint8, device=env.device)
    out_len = torch.empty(n, dtype=torch.int32, device=env.device)
    encode_call(env, frames, out, out_len)
    torch.cuda.synchronize()
    w = (int(out_len.max()) + 255) // 256 * 256
    return env, frames, out[:, :w].contiguous(), out_len


def decode_call(env, buf, ln, fmt, upsample, out, status):
    env.h.check(env.L.avsim_jpeg_decode(env.h.h, buf.data_ptr(), buf.shape[1], ln.data_ptr(), None, buf.shape[0], H, W, fmt, upsample, out.data_ptr(), status.data_ptr()))


def bench_frames(n, rounds, pool):
    import torch
    env, frames, buf, ln = streams_of(n)
    f32 = torch.empty((n, 3, H, W), dtype=torch.float32, device=env.device)
    u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=env.device)
    status = torch.empty(n, dtype=torch.int32, device=env.device)
    pin_raw = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    pin_raw.copy_(frames)
    pin_jpg = torch.empty(buf.shape, dtype=torch.uint8).pin_memory()
    pin_jpg.copy_(buf)
    pin_len = torch.empty(n, dtype=torch.int32).pin_memory()
    pin_len.copy_(ln)
    d_raw, d_jpg, d_len = torch.empty_like(frames), torch.empty_like(buf), torch.empty_like(ln)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fmt, upsample, out):
        ev[0].record(); decode_call(env, buf, ln, fmt, upsample, out, status); ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def kernels():
        """ms of the three kernels of one f32 / replicate call, from the events the call records itself."""
        import ctypes
        env.h.check(env.L.avsim_set_option(env.h.h, b"jpeg_decode_events", 1.0))
        decode_call(env, buf, ln, 1, 0, f32, status)
        ms = []
        for a in (12, 13, 14):
            v = ctypes.c_float()
            env.h.check(env.L.avsim_event_elapsed_ms(env.h.h, a, a + 1, ctypes.byref(v)))
            ms.append(v.value)
        env.h.check(env.L.avsim_set_option(env.h.h, b"jpeg_decode_events", 0.0))
        return ms

    def with_jpeg():
        d_jpg.copy_(pin_jpg, non_blocking=True)
        d_len.copy_(pin_len, non_blocking=True)
        decode_call(env, d_jpg, d_len, 1, 0, f32, status)
        torch.cuda.synchronize()

    def raw():
        d_raw.copy_(pin_raw, non_blocking=True)
        x = d_raw.permute(0, 3, 1, 2).float() / 255
        torch.cuda.synchronize()
        return x

    for _ in range(2):
        with_jpeg(); raw(); timed(1, 1, f32); timed(0, 0, u8)
    assert not bool(status.any())
    t = {"f32_replicate": [], "f32_triangle": [], "u8_replicate": [], "jpeg_path": [], "raw_path": [], "k_index": [], "k_entropy": [], "k_reconstruct": []}
    for _ in range(rounds):
        for k, v in zip(("k_index", "k_entropy", "k_reconstruct"), kernels()):
            t[k].append(v)
        t["f32_replicate"].append(timed(1, 0, f32))
        t["f32_triangle"].append(timed(1, 1, f32))
        t["u8_replicate"].append(timed(0, 0, u8))
        t0 = time.perf_counter(); with_jpeg(); t["jpeg_path"].append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter(); raw(); t["raw_path"].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in t.items()}
    lens = pin_len.numpy()
    res = {"frames": n, "height": H, "width": W, "quality": QUALITY, "stream_bytes_mean": float(lens.mean()), "stride": int(buf.shape[1]), "raw_bytes": H * W * 3,
           "decode_f32_replicate_ms": med["f32_replicate"], "decode_f32_triangle_ms": med["f32_triangle"], "decode_u8_replicate_ms": med["u8_replicate"],
           "kernel_ms_f32_replicate": {k: med[k] for k in ("k_index", "k_entropy", "k_reconstruct")},
           "decode_us_per_frame": 1e3 * med["f32_replicate"] / n, "decode_write_GBps": n * H * W * 12 / (med["f32_replicate"] * 1e-3) / 1e9,
           "streams_h2d_plus_decode_ms": med["jpeg_path"], "raw_h2d_plus_convert_ms": med["raw_path"],
           "jpeg_path_over_raw_path": med["jpeg_path"] / med["raw_path"], "all_ms": t}
    if pool is not None:
        host = [bytes(pin_jpg[i, :lens[i]].numpy()) for i in range(min(n, 256))]
        pool.map(pillow_decode, host[:32])
        t0 = time.perf_counter()
        pool.map(pillow_decode, host, chunksize=4)
        dt = time.perf_counter() - t0
        res["pillow_16_processes_frames_per_s"] = len(host) / dt
        res["device_path_frames_per_s"] = n / (med["jpeg_path"] * 1e-3)
    env.close()
    return res


def bench_record(n, parent_dir=None):
    import glob
    import shutil
    import tempfile
    from av_aloha_amd import harness
    out = {}
    for kind, kw in (("compressed", {"jpeg_quality": QUALITY}), ("raw", {})):
        d = tempfile.mkdtemp(prefix=f"record_{kind}_", dir=parent_dir)
        try:
            t0 = time.perf_counter()
            eps = harness.record_scripted("sim_slot_insertion", n, cameras=["zed_cam", "cam_left_wrist"], seed=0, stream_dir=d, **kw)
            dt = time.perf_counter() - t0
            out[kind] = {"seconds": dt, "file_bytes": sum(os.path.getsize(p) for p in glob.glob(os.path.join(d, "episode_*.hdf5"))), "episodes": len(eps)}
        finally:
            shutil.rmtree(d, ignore_errors=True)
    out["episodes_asked"] = n
    out["bytes_ratio"] = out["raw"]["file_bytes"] / max(1, out["compressed"]["file_bytes"])
    out["seconds_ratio"] = out["compressed"]["seconds"] / out["raw"]["seconds"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="256,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--decode-only", type=int, default=0, help="only decode this many frames ten times (for a kernel trace)")
    ap.add_argument("--record", type=int, default=0, help="also record this many episodes compressed and raw")
    ap.add_argument("--record-dir", default=None, help="where the recordings' temporary directories go (default: the system's)")
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pool = None
    if not args.no_pillow and not args.decode_only:          # the workers start before this process opens the GPU and never open it themselves
        import multiprocessing
        pool = multiprocessing.get_context("spawn").Pool(16)
    import torch
    torch.zeros(1, device="cuda")
    if args.decode_only:
        n = args.decode_only
        env, frames, buf, ln = streams_of(n)
        f32 = torch.empty((n, 3, H, W), dtype=torch.float32, device=env.device)
        status = torch.empty(n, dtype=torch.int32, device=env.device)
        for _ in range(10):
            decode_call(env, buf, ln, 1, 0, f32, status)
        torch.cuda.synchronize()
        env.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "frames": [bench_frames(int(n), args.rounds, pool) for n in args.frames.split(",") if n]}
    if pool is not None:
        pool.close()
        pool.join()
    if args.record:
        res["record_scripted"] = bench_record(args.record, args.record_dir)
    path = args.out or os.path.join(ROOT, "profiles", f"jpeg_decode_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items()}, indent=1))


if __name__ == "__main__":
    main()
