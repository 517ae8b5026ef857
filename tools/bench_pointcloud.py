"""What the device's point clouds (avsim_point_cloud) cost next to the same result as torch tensor ops.  Writes profiles/pointcloud_<tag>.json.

    python tools/bench_pointcloud.py --tag r18

256 and 4096 envs of slot_insertion at their reset poses, two cameras (the ZED left camera on the active-vision arm and the right wrist
camera) at 84 x 112 and at 120 x 160, synthetic depth (noise in [0.3, 1.5] from a seed, every pixel valid: the work depends on the number of
candidates, not on what the depth shows), a box that keeps roughly a quarter of the pixels (the medians of env 0's world x and y), P = 512 and
1024 points; HIP events around each way, the two ways alternating in one process after warm-up, medians over the rounds and the smallest and
largest round next to them (the spread a difference has to beat):
  (a) torch on the GPU from the same depth tensor and the same pose records: the deprojection as tensor ops, the mask, and the usual batched
      farthest point sampling loop -- P iterations of distance, minimum and argmax over ALL pixels of every env (a masked pixel's running
      distance is -1, so it is never chosen): the whole candidate set goes through HBM P times
  (b) avsim_point_cloud: the one call (pose kernel + k_pc_cloud)
The two need not select the same points (torch's argmax does not promise the first of equals), so the largest absolute xyz difference and the
share of equal indices are reported, not asserted -- tests/test_gpu_pointcloud.py compares (b) with the specification for equality.  Times are
call times from device events; they include the launches.  Candidates per env and the trips of the sampling loop (ceil(M' / 1024)) are recorded
with each case: they are what (b)'s time follows.

--abba-log FILE adds what bench.py gave alternating with the parent's build: lines "new <env-steps/s> ..." / "old <env-steps/s> ..." (the
parent's tree built next to this one), and whether this build's values lie inside the parent's own range widened by its spread.  With
--add-abba the profile of --tag (or --out) is only amended; that needs no GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMS = ["zed_cam_left", "wrist_cam_right"]
SIZES = [(84, 112), (120, 160)]
POINTS = [512, 1024]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def torch_cloud(torch, poses, depth, lo, hi, max_depth, P):
    """Way (a): (xyz [N, P, 3], index [N, P]) with plain tensor ops."""
    N, C, H, W = depth.shape
    dev = depth.device
    pc_, R, t = poses[:, :, :3], poses[:, :, 3:12].reshape(N, C, 3, 3), poses[:, :, 12]
    scale = (2.0 * t / float(H)).reshape(N, C, 1, 1)
    x = ((torch.arange(W, dtype=torch.float32, device=dev) + 0.5) - 0.5 * W).reshape(1, 1, 1, W) * scale
    y = -(((torch.arange(H, dtype=torch.float32, device=dev) + 0.5) - 0.5 * H).reshape(1, 1, H, 1) * scale)
    X, Y, Z = x * depth, y * depth, -depth
    w = torch.stack([((pc_[:, :, i, None, None] + R[:, :, i, 0, None, None] * X) + R[:, :, i, 1, None, None] * Y) + R[:, :, i, 2, None, None] * Z for i in range(3)], dim=-1)
    w = w.reshape(N, C * H * W, 3)
    mask = (depth.reshape(N, -1) < max_depth) & ((w >= lo) & (w <= hi)).all(dim=-1)
    mind = torch.where(mask, torch.full_like(w[:, :, 0], float("inf")), torch.full_like(w[:, :, 0], -1.0))
    sel = mask.to(torch.int8).argmax(dim=1)
    rows = torch.arange(N, device=dev)
    index = torch.empty((N, P), dtype=torch.int64, device=dev)
    index[:, 0] = sel
    for p in range(1, P):
        d = w - w[rows, sel][:, None, :]
        mind = torch.minimum(mind, (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2])
        sel = mind.argmax(dim=1)
        index[:, p] = sel
    return w[rows[:, None], index], index


def bench(envs, rounds, warmup, save):
    import numpy as np
    import torch
    from av_aloha_amd import pointcloud
    from av_aloha_amd.vec_env import VecEnv
    res = {"cameras": CAMS, "cases": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for N in envs:
        env = VecEnv("slot_insertion", 3, N, 100, cameras=())
        env.reset(seed=0)
        dev = env.device
        poses = env.camera_poses(CAMS)
        for H, W in SIZES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(N + H)
            depth = torch.rand((N, len(CAMS), H, W), dtype=torch.float32, device=dev, generator=gen) * 1.2 + 0.3
            w0 = pointcloud.deproject(poses[0].cpu().numpy(), depth[0].cpu().numpy()).reshape(-1, 3)
            bounds = np.array([-50, -50, -50, np.median(w0[:, 0]), np.median(w0[:, 1]), 50], dtype=np.float32)
            lo, hi = torch.from_numpy(bounds[:3]).to(dev), torch.from_numpy(bounds[3:]).to(dev)
            for P in POINTS:
                def way_a():
                    return torch_cloud(torch, poses, depth, lo, hi, pointcloud.FAR_PLANE, P)

                def way_b():
                    return env.point_cloud(CAMS, H, W, bounds, P, depth=depth)

                a, b = way_a(), way_b()
                torch.cuda.synchronize()
                count = b[2].cpu().numpy()
                diff = float((a[0] - b[0]).abs().max())
                same = float((a[1] == b[1].to(torch.int64)).float().mean())
                del a, b
                t = {"a_torch": [], "b_point_cloud": []}
                for r in range(warmup + rounds):
                    for key, way in (("a_torch", way_a), ("b_point_cloud", way_b)):
                        ev[0].record()
                        y = way()
                        ev[1].record()
                        torch.cuda.synchronize()
                        del y
                        if r >= warmup:
                            t[key].append(ev[0].elapsed_time(ev[1]))
                med = statistics.median(t["b_point_cloud"])
                key = f"{N}_envs_{H}x{W}_P{P}"
                M = count[:, 0]
                res["cases"][key] = {**{k: summary(v) for k, v in t.items()}, "envs": N, "height": H, "width": W, "points": P, "pixels_per_env": len(CAMS) * H * W,
                                     "candidates_per_env": {"min": int(M.min()), "median": float(np.median(M)), "max": int(M.max())},
                                     "sampling_trips_max": int(-(-min(int(M.max()), pointcloud.MAX_CANDIDATES) // 1024)),
                                     "a_over_b": statistics.median(t["a_torch"]) / med,
                                     "a_spread": (max(t["a_torch"]) - min(t["a_torch"])) / statistics.median(t["a_torch"]),
                                     "b_spread": (max(t["b_point_cloud"]) - min(t["b_point_cloud"])) / med,
                                     "b_us_per_env": 1e3 * med / N, "b_ns_per_env_and_selection": 1e6 * med / N / P,
                                     "max_abs_xyz_diff_from_torch": diff, "share_of_equal_indices": same}
                print(key, json.dumps(res["cases"][key]), flush=True)
                save(res)          # (after every case: a run that is cut short leaves what it measured)
            del depth
        env.close()
    return res


def abba(path):
    """{"new": [...], "old": [...], ...} of an alternating bench.py log (module docstring)."""
    runs = {"new": [], "old": []}
    with open(path) as f:
        for line in f:
            w = line.split()
            if len(w) >= 2 and w[0] in runs:
                runs[w[0]].append(float(w[1]))
    if not runs["new"] or not runs["old"]:
        raise SystemExit(f"bench_pointcloud: {path} holds no 'new' / 'old' lines")
    lo, hi = min(runs["old"]), max(runs["old"])
    return {"command": "bench.py --gpus 1 --steps 20 --warmup 5", "unit": "env-steps/s", **runs, "parent_spread": (hi - lo) / statistics.median(runs["old"]),
            "new_median_over_old_median": statistics.median(runs["new"]) / statistics.median(runs["old"]),
            "new_inside_parent_range_widened_by_its_spread": bool(lo - (hi - lo) <= min(runs["new"]) and max(runs["new"]) <= hi + (hi - lo))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    ap.add_argument("--abba-log", default=None)
    ap.add_argument("--add-abba", action="store_true")
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", f"pointcloud_{args.tag}.json")
    if args.add_abba:
        with open(path) as f:
            res = json.load(f)
        res["bench_py_alternating_with_parent"] = abba(args.abba_log)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["bench_py_alternating_with_parent"], indent=1))
        return
    if args.rounds < 20:
        raise SystemExit("bench_pointcloud: at least 20 rounds")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    name = torch.cuda.get_device_name(0)

    def save(r):
        with open(path, "w") as f:
            json.dump({"device": name, **r}, f, indent=1)

    res = {"device": name, **bench(args.envs, args.rounds, args.warmup, save)}
    if args.abba_log:
        res["bench_py_alternating_with_parent"] = abba(args.abba_log)
    save({k: v for k, v in res.items() if k != "device"})
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}, indent=1))


if __name__ == "__main__":
    main()
