"""Throughput of the device-resident vector env (av_aloha_amd/vec_env.py) against the host facade (env.make + preprocess_observation),
the episode layer's cost next to avsim_step, and k_vis_render's float32 store against its u8 one.  Writes profiles/vec_env_<tag>.json.

    python tools/bench_vec_env.py --envs 64,256,1024 --steps 20 --tag r07
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENV_ID = "gym_guided_vision/SlotInsertion-3Arms-v0"
CAMS4 = ["zed_cam_left", "zed_cam_right", "wrist_cam_left", "wrist_cam_right"]


def vec_rate(N, cams, fmt, steps, H, W):
    import torch
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(ENV_ID, N, 300, cameras=cams, obs_format=fmt, observation_height=H, observation_width=W)
    env.reset(seed=0)
    a = env._ap.float().clone()
    for _ in range(2):
        env.step(a)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        env.step(a)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    env.close()
    return N * steps / dt


def host_rate(N, cams, steps, H, W):
    import torch
    from av_aloha_amd.env import make
    from av_aloha_amd.harness import preprocess_observation
    env = make(ENV_ID, cameras=cams, num_envs=N, observation_height=H, observation_width=W)
    np.random.seed(0)
    obs, _ = env.reset()
    a = np.asarray(obs["agent_pos"], dtype=np.float32)
    dev = torch.device("cuda")
    for k in range(steps + 1):
        if k == 1:
            t = time.perf_counter()
        obs, *_ = env.step(a)
        pre = {k2: v.to(dev) for k2, v in preprocess_observation(obs).items()}      # eval.py:96-124: the observation goes to the policy's GPU
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    env.close()
    return N * steps / dt


def episode_overhead(N, steps):
    """HIP events around avsim_episode_step and around avsim_step, no cameras (ms per call)."""
    import torch
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(ENV_ID, N, 300, cameras=[])
    env.reset(seed=0)
    a = env._ap.float().clone()
    h, L = env.h, env.L
    out = {}
    for name in ("avsim_step", "avsim_episode_step", "avsim_step", "avsim_episode_step"):
        for _ in range(3):
            env.step(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            if name == "avsim_step":
                h.check(L.avsim_step(h.h, a.data_ptr(), 20, env._ap.data_ptr(), env._reward.data_ptr(), env._success.data_ptr()))
            else:
                h.check(L.avsim_episode_step(h.h, a.data_ptr(), 20, env._ap.data_ptr(), env._reward.data_ptr(), env._success.data_ptr(),
                                             env._term.data_ptr(), env._trunc.data_ptr(), env._id.data_ptr(), env._elapsed.data_ptr()))
        e1.record()
        e1.synchronize()
        out.setdefault(name, []).append(e0.elapsed_time(e1) / steps)
    env.close()
    r = {k: min(v) for k, v in out.items()}
    r["overhead_pct"] = 100.0 * (r["avsim_episode_step"] / r["avsim_step"] - 1.0)
    return r


def render_f32_vs_u8(N, H, W, reps):
    import torch
    from av_aloha_amd.vec_env import make_vec
    ids = None
    res = {}
    for fmt in ("gym", "lerobot", "gym", "lerobot"):
        env = make_vec(ENV_ID, N, 300, cameras=CAMS4, obs_format=fmt, observation_height=H, observation_width=W)
        env.reset(seed=0)
        env._obs()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            env._obs()        # the state does not change: the pose pass and the shadow maps are skipped, k_vis_render alone runs
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
        res.setdefault(fmt, []).append(ms)
        env.close()
    out = {"u8_ms": min(res["gym"]), "f32_ms": min(res["lerobot"])}
    px = N * len(CAMS4) * H * W
    out["u8_write_GBps"] = px * 3 / out["u8_ms"] / 1e6
    out["f32_write_GBps"] = px * 12 / out["f32_ms"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,256,1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--max-camera-envs", type=int, default=256, help="largest batch run with 4 cameras (1024 x 4 x 480 x 640 f32 = 15 GB)")
    ap.add_argument("--tag", default="latest")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    H, W = a.height, a.width
    rows = []
    for N in [int(x) for x in a.envs.split(",")]:
        for cams in ([], CAMS4):
            if cams and N > a.max_camera_envs:
                continue
            r = {"num_envs": N, "cameras": len(cams), "H": H, "W": W}
            r["vec_lerobot_env_steps_s"] = vec_rate(N, cams, "lerobot", a.steps, H, W)
            r["vec_gym_env_steps_s"] = vec_rate(N, cams, "gym", a.steps, H, W)
            if not a.skip_host:
                r["host_env_preprocess_env_steps_s"] = host_rate(N, cams, max(2, a.steps // 4 if cams else a.steps), H, W)
                r["speedup_lerobot"] = r["vec_lerobot_env_steps_s"] / r["host_env_preprocess_env_steps_s"]
            print(json.dumps(r), flush=True)
            rows.append(r)
    res = {"rows": rows, "episode_layer_4096": episode_overhead(4096, 20), "render_256x4": render_f32_vs_u8(256, H, W, 5)}
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"vec_env_{a.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(path)


if __name__ == "__main__":
    main()
