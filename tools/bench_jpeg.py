"""What the device JPEG encoder (avsim_jpeg_encode) costs and what it saves.  Writes profiles/jpeg_<tag>.json.

    python tools/bench_jpeg.py --frames 64,256,1024 --tag r08
    rocprofv3 --kernel-trace --stats -d trace -- python tools/bench_jpeg.py --encode-only 256     # kernel times, in a run of its own

* encode: HIP events around avsim_jpeg_encode of n rendered 480 x 640 frames (SlotInsertion, zed_cam_left, u8) at quality 90; the
  read bandwidth is n x H x W x 3 bytes over that time.
* frames out of the GPU: encode + copy of the streams to pinned host memory (the lengths first, then as many bytes per stream as the
  longest one has -- what harness.evaluate_vec does) against the copy of the same raw u8 frames to pinned host memory.  The two sides
  alternate in one process; medians over the rounds.
* evaluate_vec at 256 envs with one 480 x 640 camera, with video_episodes=16 and without, alternating.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENV_ID = "gym_guided_vision/SlotInsertion-3Arms-v0"
H, W, QUALITY = 480, 640, 90


def rendered_frames(n):
    """u8 [n, H, W, 3] on the device: the zed_cam_left images of min(n, 256) envs over successive steps of a wiggle."""
    import torch
    from av_aloha_amd.vec_env import make_vec
    N = min(n, 256)
    env = make_vec(ENV_ID, N, 300, cameras=["zed_cam_left"], obs_format="gym", observation_height=H, observation_width=W)
    obs, _ = env.reset(seed=0)
    a = env._ap.float().clone()
    parts = []
    while sum(p.shape[0] for p in parts) < n:
        a[:, :6] += 0.05
        obs, *_ = env.step(a)
        parts.append(obs["pixels"]["zed_cam_left"].clone())
    torch.cuda.synchronize()
    return env, torch.cat(parts)[:n].contiguous()


def encode_call(env, frames, out, out_len):
    env.h.check(env.L.avsim_jpeg_encode(env.h.h, frames.data_ptr(), 0, None, frames.shape[0], H, W, QUALITY, out.data_ptr(), out.shape[1], out_len.data_ptr()))


def bench_frames(n, rounds):
    import torch
    env, frames = rendered_frames(n)
    stride = 128 << 10                    # four times a quality-90 frame; VecEnv.jpeg_stride() reserves more
    out = torch.empty((n, stride), dtype=torch.uint8, device=env.device)
    out_len = torch.empty(n, dtype=torch.int32, device=env.device)
    pin_raw = torch.empty(frames.shape, dtype=torch.uint8).pin_memory()
    pin_jpg = torch.empty((n, stride), dtype=torch.uint8).pin_memory()
    pin_len = torch.empty(n, dtype=torch.int32).pin_memory()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def with_jpeg():
        encode_call(env, frames, out, out_len)
        pin_len.copy_(out_len, non_blocking=True)
        torch.cuda.synchronize()
        w = int(pin_len.max())
        pin_jpg[:, :w].copy_(out[:, :w], non_blocking=True)
        torch.cuda.synchronize()
        return w

    def raw():
        pin_raw.copy_(frames, non_blocking=True)
        torch.cuda.synchronize()

    for _ in range(2):
        with_jpeg(); raw()
    t_enc, t_jpg, t_raw = [], [], []
    for _ in range(rounds):
        ev[0].record(); encode_call(env, frames, out, out_len); ev[1].record()
        torch.cuda.synchronize()
        t_enc.append(ev[0].elapsed_time(ev[1]))
        t = time.perf_counter(); with_jpeg(); t_jpg.append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter(); raw(); t_raw.append(1e3 * (time.perf_counter() - t))
    lens = pin_len.numpy()
    med = statistics.median
    res = {"frames": n, "height": H, "width": W, "quality": QUALITY, "stream_bytes_mean": float(lens.mean()), "stream_bytes_max": int(lens.max()),
           "raw_bytes": H * W * 3, "encode_ms": med(t_enc), "encode_us_per_frame": 1e3 * med(t_enc) / n,
           "encode_read_GBps": n * H * W * 3 / (med(t_enc) * 1e-3) / 1e9, "encode_plus_copy_ms": med(t_jpg), "raw_copy_ms": med(t_raw),
           "raw_copy_GBps": n * H * W * 3 / (med(t_raw) * 1e-3) / 1e9, "encode_plus_copy_over_raw_copy": med(t_jpg) / med(t_raw),
           "encode_ms_all": t_enc, "encode_plus_copy_ms_all": t_jpg, "raw_copy_ms_all": t_raw}
    env.close()
    return res


def bench_evaluate(num_envs, steps, video_episodes, rounds):
    import torch
    from av_aloha_amd.harness import evaluate_vec
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(ENV_ID, num_envs, steps, cameras=["zed_cam_left"], obs_format="lerobot", observation_height=H, observation_width=W)
    base = []

    def policy(obs, info):
        if not base:
            base.append(env._ap.float().clone())
        return base[0]
    times = {"video": [], "plain": []}
    with tempfile.TemporaryDirectory() as d:
        evaluate_vec(env, policy, num_envs, video_dir=d, video_episodes=video_episodes)          # warm-up of both paths
        for _ in range(rounds):
            for kind in ("video", "plain"):
                torch.cuda.synchronize()
                t = time.perf_counter()
                evaluate_vec(env, policy, num_envs, **({"video_dir": d, "video_episodes": video_episodes} if kind == "video" else {}))
                torch.cuda.synchronize()
                times[kind].append(time.perf_counter() - t)
        size = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    env.close()
    med = statistics.median
    return {"num_envs": num_envs, "max_episode_steps": steps, "video_episodes": video_episodes, "seconds_video": med(times["video"]),
            "seconds_plain": med(times["plain"]), "video_over_plain": med(times["video"]) / med(times["plain"]), "avi_bytes": size,
            "seconds_video_all": times["video"], "seconds_plain_all": times["plain"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="64,256,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--eval-steps", type=int, default=20)
    ap.add_argument("--encode-only", type=int, default=0, help="only encode this many frames ten times (for a kernel trace)")
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    if args.encode_only:
        env, frames = rendered_frames(args.encode_only)
        out = torch.empty((args.encode_only, env.jpeg_stride(QUALITY)), dtype=torch.uint8, device=env.device)
        out_len = torch.empty(args.encode_only, dtype=torch.int32, device=env.device)
        for _ in range(10):
            encode_call(env, frames, out, out_len)
        torch.cuda.synchronize()
        env.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "frames": [bench_frames(int(n), args.rounds) for n in args.frames.split(",")]}
    if args.eval_envs:
        res["evaluate_vec"] = bench_evaluate(args.eval_envs, args.eval_steps, 16, 3)
    path = args.out or os.path.join(ROOT, "profiles", f"jpeg_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items()}, indent=1))


if __name__ == "__main__":
    main()
