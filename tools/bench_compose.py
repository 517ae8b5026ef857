"""What the device's composer (avsim_compose, csrc/avsim_compose.hip.h) costs.  Writes profiles/compose_<tag>.json.

    python tools/bench_compose.py --tag r10
    python tools/bench_compose.py --sections kernel --tag dev

* kernel: HIP events around avsim_compose for (a) 256 frames of three 480 x 640 cameras side by side in a 480 x 1920 canvas (sizes equal: a
  copy) and (b) 256 frames shrunk to the 120 x 160 cells of one 16 x 16 grid; bytes read plus written over that time, next to the rate of
  a device-to-device copy (hipMemcpyAsync through torch's copy_) of buffers of the same sizes measured in the same process, and next to the same two composites in
  torch (float conversion, torch.nn.functional.interpolate(mode="bilinear", antialias=True) per camera, slice assignment, back to u8).
  The sides alternate in one process; medians over the rounds.
* dataset: harness.visualize_dataset over 32 compressed episodes recorded with record_scripted(jpeg_quality=90), device path: frames per
  second and the bytes that crossed the bus.  (The host path is for tests and small files and is not timed at this size.)
* evaluate: evaluate_vec at 256 envs with grid_video (grid_envs=64) and without, alternating.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENV_ID = "gym_guided_vision/SlotInsertion-3Arms-v0"
H, W = 480, 640
med = statistics.median


def event_ms(fn, torch):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); fn(); ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def bench_kernel(rounds, frames):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from av_aloha_amd.compose import layout_grid
    from av_aloha_amd.vec_env import VecEnv
    env = VecEnv("insert_peg", 3, 1, 1)
    dev = env.device
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    # (a) three cameras side by side, sizes equal
    cams = [torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(3)]
    canvas = torch.zeros((frames, H, 3 * W, 3), dtype=torch.uint8, device=dev)
    places = [np.array([(i, i, c * W, 0, W, H) for i in range(frames)], np.int32) for c in range(3)]
    copy_dst = torch.empty_like(canvas).view(3, frames, H, W, 3)

    def ours_row():
        for c in range(3):
            env.compose(cams[c], places[c], out=canvas)

    def memcpy_row():
        for c in range(3):
            copy_dst[c].copy_(cams[c])

    tcanvas = torch.zeros_like(canvas)

    def torch_row():
        for c in range(3):
            x = F.interpolate(cams[c].permute(0, 3, 1, 2).float(), size=(H, W), mode="bilinear", antialias=True)
            tcanvas[:, :, c * W:(c + 1) * W] = x.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)

    # (b) a 16 x 16 grid of 120 x 160 cells
    rows, GH, GW = layout_grid(frames, 120, 160, cols=16)
    gplaces = np.array([(0, i, x0, y0, w, h) for i, (x0, y0, w, h) in enumerate(rows)], np.int32)
    grid = torch.zeros((1, GH, GW, 3), dtype=torch.uint8, device=dev)
    tgrid = torch.zeros_like(grid)
    gcopy_src = torch.empty(frames * H * W * 3 + GH * GW * 3, dtype=torch.uint8, device=dev)      # read + written bytes of (b), halved below
    gcopy_dst = torch.empty_like(gcopy_src)

    def ours_grid():
        env.compose(cams[0], gplaces, out=grid)

    def memcpy_grid():
        n = gcopy_src.numel() // 2
        gcopy_dst[:n].copy_(gcopy_src[:n])

    def torch_grid():
        x = F.interpolate(cams[0].permute(0, 3, 1, 2).float(), size=(120, 160), mode="bilinear", antialias=True)
        x = x.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
        tgrid[0] = x.reshape(GH // 120, GW // 160, 120, 160, 3).permute(0, 2, 1, 3, 4).reshape(GH, GW, 3)

    sides = {"row": (ours_row, memcpy_row, torch_row, 2 * 3 * frames * H * W * 3), "grid": (ours_grid, memcpy_grid, torch_grid, frames * H * W * 3 + GH * GW * 3)}
    for name, (ours, cp, tt, nbytes) in sides.items():
        for _ in range(2):
            ours(); cp(); tt()
        torch.cuda.synchronize()
        t = {"compose": [], "memcpy": [], "torch": []}
        for _ in range(rounds):
            t["compose"].append(event_ms(ours, torch))
            t["memcpy"].append(event_ms(cp, torch))
            t["torch"].append(event_ms(tt, torch))
        a, b = (canvas, tcanvas) if name == "row" else (grid, tgrid)
        diff = (a.int() - b.int()).abs()
        out[name] = {"frames": frames, "bytes_read_plus_written": nbytes, "compose_ms": med(t["compose"]), "compose_GBps": nbytes / (med(t["compose"]) * 1e-3) / 1e9,
                     "memcpy_d2d_ms": med(t["memcpy"]), "memcpy_d2d_GBps_read_plus_written": nbytes / (med(t["memcpy"]) * 1e-3) / 1e9,
                     "torch_ms": med(t["torch"]), "torch_over_compose": med(t["torch"]) / med(t["compose"]),
                     "max_abs_difference_to_torch": int(diff.max()), "compose_ms_all": t["compose"], "memcpy_d2d_ms_all": t["memcpy"], "torch_ms_all": t["torch"]}
    env.close()
    return out


def bench_dataset(episodes, workdir):
    from av_aloha_amd import harness
    d = os.path.join(workdir, "set")
    t = time.perf_counter()
    harness.record_scripted("sim_insert_peg", episodes, cameras=["zed_cam", "cam_left_wrist"], seed=0, stream_dir=d, jpeg_quality=90, keep_diverged=True)
    t_record = time.perf_counter() - t
    paths = sorted(glob.glob(os.path.join(d, "episode_*.hdf5")))
    file_bytes = sum(os.path.getsize(p) for p in paths)
    res = harness.visualize_dataset(paths, os.path.join(workdir, "all.avi"), stride=20)           # warm-up: tables, staging
    res = harness.visualize_dataset(paths, os.path.join(workdir, "all.avi"), stride=20)
    every = harness.visualize_dataset(paths, os.path.join(workdir, "every.avi"), stride=1)
    return {"episodes": len(paths), "record_seconds": t_record, "dataset_file_bytes": file_bytes,
            "stride_20": {k: res[k] for k in ("frames", "seconds", "bytes_to_device", "bytes_from_device")} | {"frames_per_second": res["frames"] / res["seconds"]},
            "stride_1": {k: every[k] for k in ("frames", "seconds", "bytes_to_device", "bytes_from_device")} | {"frames_per_second": every["frames"] / every["seconds"],
                                                                                                            "avi_bytes": os.path.getsize(os.path.join(workdir, "every.avi"))},
            "note": "seconds include reading and parsing the episode files on the host"}


def bench_evaluate(num_envs, steps, grid_envs, rounds, workdir):
    import torch
    from av_aloha_amd.harness import evaluate_vec
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(ENV_ID, num_envs, steps, cameras=["zed_cam_left"], obs_format="lerobot", observation_height=H, observation_width=W)
    base = []

    def policy(obs, info):
        if not base:
            base.append(env._ap.float().clone())
        return base[0]
    path = os.path.join(workdir, "grid.avi")
    kw = {"grid_video": path, "grid_envs": grid_envs}
    times = {"grid": [], "plain": []}
    evaluate_vec(env, policy, num_envs, **kw)          # warm-up of both paths
    for _ in range(rounds):
        for kind in ("grid", "plain"):
            torch.cuda.synchronize()
            t = time.perf_counter()
            evaluate_vec(env, policy, num_envs, **(kw if kind == "grid" else {}))
            torch.cuda.synchronize()
            times[kind].append(time.perf_counter() - t)
    size = os.path.getsize(path)
    env.close()
    return {"num_envs": num_envs, "max_episode_steps": steps, "grid_envs": grid_envs, "seconds_grid": med(times["grid"]), "seconds_plain": med(times["plain"]),
            "overhead_percent": 100 * (med(times["grid"]) / med(times["plain"]) - 1), "avi_bytes": size, "seconds_grid_all": times["grid"],
            "seconds_plain_all": times["plain"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernel,dataset,evaluate")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--eval-steps", type=int, default=20)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    res = {"device": torch.cuda.get_device_name(0)}
    sections = args.sections.split(",")
    with tempfile.TemporaryDirectory() as d:
        if "kernel" in sections:
            res["kernel"] = bench_kernel(args.rounds, args.frames)
        if "dataset" in sections:
            res["visualize_dataset"] = bench_dataset(args.episodes, d)
        if "evaluate" in sections:
            res["evaluate_vec"] = bench_evaluate(args.eval_envs, args.eval_steps, 64, 3, d)
    path = args.out or os.path.join(ROOT, "profiles", f"compose_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
