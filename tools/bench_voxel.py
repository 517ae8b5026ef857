"""What the device's voxel grids (avsim_voxel_grid) cost next to the same result as torch tensor ops.  Writes profiles/voxel_<tag>.json.

    python tools/bench_voxel.py --tag r19

256 and 1024 envs of slot_insertion at their reset poses, three cameras (the ZED left camera and the two wrist cameras) at 84 x 112, the
depth and the u8 colour images rendered once, the workspace box BOUNDS, grids 32^3 and 64^3, with and without colour; HIP events around each
way, the three ways alternating in one process after warm-up, medians over the rounds and the smallest and largest round next to them (the
spread a difference has to beat):
  (a) torch on the GPU from the same depth, colour and pose tensors: the specification's formulas as tensor ops -- deprojection, mask, cell
      and position in 1/256 --, seven (four without colour) index_add_ calls on float32 and the division; a pixel that is no candidate
      adds 0 at the cell its clamped coordinates name, so the adds are spread like the candidates' and nothing synchronises
  (b) avsim_voxel_grid as the library was built: the pose kernel, clear, accumulate, finish
  (c) the same call with the OTHER accumulate form (option "voxel_other_form"; which form ships is the build's AVSIM_VOXEL_MERGE, 1 =
      merged unless built otherwise -- the tool does not know it and does not need to)
Conditions (asserted at the end, after the profile is written): the median of (b) is below the fastest round of (a) in every case, and (b)
is not slower than (c) beyond the two forms' own round-to-round spread.  (b) and (c) give the same bits (integer sums; asserted).  (a) sums
floats in arrival order: its largest difference from (b) is reported, not asserted.  With each case: the bytes the three passes move and the
time they would take (with the merged form's added bytes) at the HBM roof (6.29 TB/s measured copy rate of the part, 8 TB/s nominal), the atomic wave-instructions and the lane
adds of both forms, and the mean length of the runs the merge found -- all computed from the cells of the candidates with tensor ops, in the
kernel's own assignment of pixels to waves (256 consecutive pixels of an env per workgroup).

--abba-log FILE adds what bench.py gave alternating with the parent's build: lines "new <env-steps/s> ..." / "old <env-steps/s> ..."; with
--add-abba the profile of --tag (or --out) is only amended, which needs no GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CAMS = ["zed_cam_left", "wrist_cam_left", "wrist_cam_right"]
H, W = 84, 112
BOUNDS = (-0.6, -0.5, -0.05, 0.6, 0.7, 0.8)
GRIDS = [32, 64]
HBM_MEASURED, HBM_NOMINAL = 6.29e12, 8.0e12


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def torch_cells(torch, poses, depth, lo, hi, max_depth, g):
    """(mask [N, Q], flat cell int64 [N, Q], q float32 [N, Q, 3], i float32 [N, Q, 3]) with plain tensor ops: the specification's formulas."""
    N, C, Hh, Ww = depth.shape
    dev = depth.device
    pc_, R, t = poses[:, :, :3], poses[:, :, 3:12].reshape(N, C, 3, 3), poses[:, :, 12]
    scale = (2.0 * t / float(Hh)).reshape(N, C, 1, 1)
    x = ((torch.arange(Ww, dtype=torch.float32, device=dev) + 0.5) - 0.5 * Ww).reshape(1, 1, 1, Ww) * scale
    y = -(((torch.arange(Hh, dtype=torch.float32, device=dev) + 0.5) - 0.5 * Hh).reshape(1, 1, Hh, 1) * scale)
    X, Y, Z = x * depth, y * depth, -depth
    w = torch.stack([((pc_[:, :, i, None, None] + R[:, :, i, 0, None, None] * X) + R[:, :, i, 1, None, None] * Y) + R[:, :, i, 2, None, None] * Z for i in range(3)], dim=-1)
    w = w.reshape(N, C * Hh * Ww, 3)
    mask = (depth.reshape(N, -1) < max_depth) & ((w >= lo) & (w <= hi)).all(dim=-1)
    gf = torch.full((3,), float(g), dtype=torch.float32, device=dev)
    u = (w - lo) * (gf / (hi - lo))
    i = torch.minimum(torch.floor(u), gf - 1.0).clamp_(min=0.0).nan_to_num_(nan=0.0)          # (clamped: a pixel outside the box names a cell too)
    q = ((u - i) * 256.0).to(torch.int32).clamp_(0, 255).to(torch.float32)
    ii = i.to(torch.int64)
    return mask, (ii[:, :, 0] * g + ii[:, :, 1]) * g + ii[:, :, 2], q, i


def torch_grid(torch, poses, depth, rgb, lo, hi, max_depth, g):
    """Way (a): float32 [N, g, g, g, 8]."""
    N = depth.shape[0]
    dev = depth.device
    cells = g * g * g
    mask, flat, q, _ = torch_cells(torch, poses, depth, lo, hi, max_depth, g)
    # a pixel that is no candidate adds 0 at the cell its clamped coordinates name: no compaction (that would synchronise), and no cell that
    # every such pixel aims at (one shared dump cell serialises a third of the adds on one address)
    idx = (flat + torch.arange(N, device=dev)[:, None] * cells).reshape(-1)
    m = mask.reshape(-1).to(torch.float32)
    acc = torch.zeros((7, N * cells), dtype=torch.float32, device=dev)
    acc[0].index_add_(0, idx, m)
    for k in range(3):
        acc[1 + k].index_add_(0, idx, q[:, :, k].reshape(-1) * m)
    if rgb is not None:
        c = rgb.reshape(-1, 3).to(torch.float32)
        for k in range(3):
            acc[4 + k].index_add_(0, idx, c[:, k] * m)
    acc = acc.reshape(7, N, g, g, g)
    n = acc[0]
    occ = n > 0
    safe = torch.where(occ, n, torch.ones_like(n))
    size = (hi - lo) / float(g)
    out = torch.zeros((N, g, g, g, 8), dtype=torch.float32, device=dev)
    ar = torch.arange(g, dtype=torch.float32, device=dev)
    for k in range(3):
        ik = ar.reshape([1] + [g if j == k else 1 for j in range(3)])
        out[..., k] = torch.where(occ, lo[k] + (ik + (acc[1 + k] / safe + 0.5) * (1.0 / 256.0)) * size[k], torch.zeros_like(n))
        out[..., 3 + k] = (acc[4 + k] / safe) * (1.0 / 255.0)
    out[..., 6] = n
    out[..., 7] = occ.to(torch.float32)
    return out


def run_statistics(torch, mask, flat, nwords):
    """The accumulate pass in numbers, from the candidates' cells in the kernel's own lanes: 256 consecutive pixels of an env per workgroup."""
    N, Q = flat.shape
    pad = (-Q) % 256
    key = torch.where(mask, flat, torch.full_like(flat, -1))
    if pad:
        key = torch.cat([key, torch.full((N, pad), -1, dtype=key.dtype, device=key.device)], dim=1)
    key = key.reshape(N, -1, 64)
    head = torch.ones_like(key, dtype=torch.bool)
    head[:, :, 1:] = key[:, :, 1:] != key[:, :, :-1]
    valid = key >= 0
    runs = int((head & valid).sum())
    cand = int(valid.sum())
    waves = int(valid.any(dim=2).sum())
    return {"candidates": cand, "runs": runs, "mean_run_length": cand / max(runs, 1), "waves_that_add": waves, "atomic_wave_instructions": waves * nwords,
            "lane_adds_merged": runs * nwords, "lane_adds_plain": cand * nwords}


def bench(envs, rounds, warmup, save):
    import numpy as np
    import torch
    from av_aloha_amd import pointcloud
    from av_aloha_amd.vec_env import VecEnv
    res = {"cameras": CAMS, "height": H, "width": W, "bounds": list(BOUNDS), "cases": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    bounds = np.array(BOUNDS, dtype=np.float32)
    for N in envs:
        env = VecEnv("slot_insertion", 3, N, 100, cameras=())
        env.reset(seed=0)
        dev = env.device
        poses = env.camera_poses(CAMS)
        ids = np.array([env.manifest["camera_names"].index(c) for c in CAMS], dtype=np.int32)
        depth = torch.empty((N, len(CAMS), H, W), dtype=torch.float32, device=dev)
        rgb8 = torch.empty((N, len(CAMS), H, W, 3), dtype=torch.uint8, device=dev)
        env.h.check(env.L.avsim_render_depth(env.h.h, ids.ctypes.data, len(ids), H, W, depth.data_ptr()))
        env.h.check(env.L.avsim_render_rgb(env.h.h, ids.ctypes.data, len(ids), H, W, rgb8.data_ptr()))
        lo, hi = torch.from_numpy(bounds[:3]).to(dev), torch.from_numpy(bounds[3:]).to(dev)

        def other_form(on):
            env.h.check(env.L.avsim_set_option(env.h.h, b"voxel_other_form", 1.0 if on else 0.0))

        for g in GRIDS:
            for colour in (False, True):
                rgb = rgb8 if colour else None
                out_b = torch.empty((N, g, g, g, 8), dtype=torch.float32, device=dev)
                out_c = torch.empty_like(out_b)

                def way_a():
                    return torch_grid(torch, poses, depth, rgb, lo, hi, pointcloud.FAR_PLANE, g)

                def way_b():
                    return env.voxel_grid(CAMS, H, W, bounds, g, depth=depth, rgb=rgb, out=out_b)

                def way_c():
                    other_form(True)
                    r = env.voxel_grid(CAMS, H, W, bounds, g, depth=depth, rgb=rgb, out=out_c)
                    other_form(False)
                    return r

                a, b, c = way_a(), way_b(), way_c()
                torch.cuda.synchronize()
                assert torch.equal(b.view(torch.int32), c.view(torch.int32)), "the two accumulate forms differ"
                diff_pos = float((a[..., :3] - b[..., :3]).abs().max())
                diff_pos_cells = float(((a[..., :3] - b[..., :3]).abs() / ((hi - lo) / g)).max())
                diff_col = float((a[..., 3:6] - b[..., 3:6]).abs().max())
                same_counts = bool(torch.equal(a[..., 6:], b[..., 6:]))
                occupied = int((b[..., 7] > 0).sum())
                mask, flat, _, _ = torch_cells(torch, poses, depth, lo, hi, pointcloud.FAR_PLANE, g)
                nwords = 7 if colour else 4
                stats = run_statistics(torch, mask, flat, nwords)
                del a, mask, flat
                t = {"a_torch": [], "b_shipped": [], "c_other_form": []}
                for r in range(warmup + rounds):
                    for key, way in (("a_torch", way_a), ("b_shipped", way_b), ("c_other_form", way_c)):
                        ev[0].record()
                        y = way()
                        ev[1].record()
                        torch.cuda.synchronize()
                        del y
                        if r >= warmup:
                            t[key].append(ev[0].elapsed_time(ev[1]))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = {k: max(v) - min(v) for k, v in t.items()}
                cells = N * g ** 3
                Q = N * len(CAMS) * H * W
                moved = {"clear_write": 32 * cells, "accumulate_read": Q * (7 if colour else 4), "finish_read": 32 * cells, "finish_write": 32 * occupied}
                added = {"accumulate_added_merged": 4 * stats["lane_adds_merged"], "accumulate_added_plain": 4 * stats["lane_adds_plain"]}
                total = sum(moved.values()) + added["accumulate_added_merged"]          # (the roof: with the fewer added bytes, whichever form ran)
                key = f"{N}_envs_grid{g}_{'colour' if colour else 'depth_only'}"
                res["cases"][key] = {**{k: summary(v) for k, v in t.items()}, "envs": N, "grid": g, "colour": colour, "pixels": Q, "cells": cells, "occupied_cells": occupied,
                                     "a_min_over_b_median": min(t["a_torch"]) / med["b_shipped"],
                                     "b_median_below_a_min": bool(med["b_shipped"] < min(t["a_torch"])),
                                     "b_minus_c_median_ms": med["b_shipped"] - med["c_other_form"], "b_c_spread_ms": max(spread["b_shipped"], spread["c_other_form"]),
                                     "b_not_slower_than_c_beyond_spread": bool(med["b_shipped"] - med["c_other_form"] <= max(spread["b_shipped"], spread["c_other_form"])),
                                     "bytes": {**moved, **added, "total_with_merged_adds": total}, "ms_at_hbm_measured_6.29TBps": 1e3 * total / HBM_MEASURED, "ms_at_hbm_nominal_8TBps": 1e3 * total / HBM_NOMINAL,
                                     "share_of_hbm_measured_roof": (1e3 * total / HBM_MEASURED) / med["b_shipped"], "accumulate": stats,
                                     "max_abs_position_diff_from_torch_m": diff_pos, "max_position_diff_from_torch_cells": diff_pos_cells, "max_abs_colour_diff_from_torch": diff_col,
                                     "counts_and_occupancy_equal_torch": same_counts}
                print(key, json.dumps(res["cases"][key]), flush=True)
                save(res)          # (after every case: a run that is cut short leaves what it measured)
                del out_b, out_c, b, c
        env.close()
    return res


def abba(path):
    from bench_pointcloud import abba as f
    return f(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    ap.add_argument("--abba-log", default=None)
    ap.add_argument("--add-abba", action="store_true")
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", f"voxel_{args.tag}.json")
    if args.add_abba:
        with open(path) as f:
            res = json.load(f)
        res["bench_py_alternating_with_parent"] = abba(args.abba_log)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["bench_py_alternating_with_parent"], indent=1))
        return
    if args.rounds < 20:
        raise SystemExit("bench_voxel: at least 20 rounds")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel: no GPU -- the measurement has no CPU form")
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
    bad = [k for k, c in res["cases"].items() if not (c["b_median_below_a_min"] and c["b_not_slower_than_c_beyond_spread"])]
    print(json.dumps({k: v for k, v in res.items() if k != "cases"}, indent=1))
    if bad:
        raise SystemExit(f"bench_voxel: the conditions do not hold in {bad}")


if __name__ == "__main__":
    main()
