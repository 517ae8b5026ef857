"""What the label image (avsim_render_labels) costs next to the depth image of the same cast.  Writes profiles/segment_<tag>.json.

    python tools/bench_segment.py --tag r21

1024 envs of slot_insertion at their reset poses (--envs), two shapes: three cameras (the ZED left camera and the two wrist cameras) at
84 x 112 -- the README's cloud shape -- and four cameras at 480 x 640.  Per shape, alternating in one process after warm-up:
  depth            avsim_render_depth
  labels_depth     avsim_render_labels, class table, depth and labels
  labels_only      avsim_render_labels, class table, labels alone
  labels_depth_8r  labels_depth with option "render_labels_form" 1: a lane's eight winners in eight registers instead of two (4 waves per
                   SIMD instead of 5; the same images, asserted)
For every way two figures per round: the image kernel alone (k_render_depth's mode, option "kernel_timing" / avsim_render_kernel_time) and
the whole call between two HIP events on the stream (pose pass, set-up kernels, staging).  Medians over the rounds, the smallest and the
largest round next to them: the spread a difference has to beat.  No ratio is asserted -- the file records labels-call / depth-call.

The parent commit has no label image: --depth-only measures avsim_render_depth alone, and --root DIR loads the package of another tree (a
checkout of the parent, built), so that

    python tools/bench_segment.py --root ../parent --depth-only --out parent.json
    python tools/bench_segment.py --tag r21 --parent-json parent.json [--parent-json parent2.json ...]

records the depth call of this build against the parent's: expected inside the runs' own spread, since the depth and colour modes
compile to what they compiled to before."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {"cloud_3cams_84x112": (["zed_cam_left", "wrist_cam_left", "wrist_cam_right"], 84, 112),
          "full_4cams_480x640": (["zed_cam_left", "zed_cam_right", "wrist_cam_left", "wrist_cam_right"], 480, 640)}


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def bench(N, rounds, warmup, depth_only, save):
    import ctypes
    import numpy as np
    import torch
    from av_aloha_amd.vec_env import VecEnv
    env = VecEnv("slot_insertion", 3, N, 100, cameras=())
    env.reset(seed=0)
    L, h, dev = env.L, env.h.h, env.device
    env.h.check(L.avsim_set_option(h, b"kernel_timing", 1.0))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"envs": N, "shapes": {}}

    def kernel_ms():
        ms, n = ctypes.c_double(0), ctypes.c_int64(0)
        env.h.check(L.avsim_render_kernel_time(h, 1, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value

    for name, (cams, H, W) in SHAPES.items():
        ids = np.array([env.manifest["camera_names"].index(c) for c in cams], dtype=np.int32)
        shape = (N, len(cams), H, W)
        depth = torch.empty(shape, dtype=torch.float32, device=dev)
        ways = {"depth": lambda: env.h.check(L.avsim_render_depth(h, ids.ctypes.data, len(ids), H, W, depth.data_ptr()))}
        if not depth_only:
            table = env.label_table("class")[0]
            labels, depth2 = torch.empty(shape, dtype=torch.uint8, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)

            def form(eight):
                env.h.check(L.avsim_set_option(h, b"render_labels_form", 1.0 if eight else 0.0))

            def labels_call(d, l, eight=False):
                form(eight)
                env.h.check(L.avsim_render_labels(h, ids.ctypes.data, len(ids), H, W, table.ctypes.data, None, d, l))
                form(False)

            ways["labels_depth"] = lambda: labels_call(depth2.data_ptr(), labels.data_ptr())
            ways["labels_only"] = lambda: labels_call(None, labels.data_ptr())
            ways["labels_depth_8r"] = lambda: labels_call(depth2.data_ptr(), labels.data_ptr(), True)
            ways["depth"]()
            ways["labels_depth"]()
            packed = labels.clone()
            assert torch.equal(depth, depth2), "the labels mode's depth is not avsim_render_depth's"
            ways["labels_depth_8r"]()
            assert torch.equal(labels, packed) and torch.equal(depth, depth2), "the two register forms differ"
        t = {k: {"kernel": [], "call": []} for k in ways}
        for r in range(warmup + rounds):
            for key, way in ways.items():
                kernel_ms()
                ev[0].record()
                way()
                ev[1].record()
                torch.cuda.synchronize()
                if r >= warmup:
                    t[key]["kernel"].append(kernel_ms())
                    t[key]["call"].append(ev[0].elapsed_time(ev[1]))
        px = N * len(cams) * H * W
        case = {"cameras": cams, "height": H, "width": W, "pixels": px, **{k: {"kernel": summary(v["kernel"]), "call": summary(v["call"])} for k, v in t.items()}}
        if not depth_only:
            for what in ("kernel", "call"):
                d = case["depth"][what]["median_ms"]
                case[f"{what}_ratio_to_depth"] = {k: case[k][what]["median_ms"] / d for k in ways if k != "depth"}
            case["bytes_written"] = {"depth": 4 * px, "labels_depth": 5 * px, "labels_only": px}
        res["shapes"][name] = case
        print(name, json.dumps(case), flush=True)
        save(res)
        del depth
    env.close()
    return res


def against_parent(res, parents):
    """The depth call of this build against the parent's runs: medians, and whether they differ by more than the runs' own spread."""
    out = {}
    for name, case in res["shapes"].items():
        for what in ("kernel", "call"):
            mine = case["depth"][what]
            theirs = [p["shapes"][name]["depth"][what] for p in parents]
            pm = statistics.median(x["median_ms"] for x in theirs)
            spread = max([mine["max_ms"] - mine["min_ms"]] + [x["max_ms"] - x["min_ms"] for x in theirs] + [max(x["median_ms"] for x in theirs) - min(x["median_ms"] for x in theirs)])
            out[f"{name}_{what}"] = {"this_build_median_ms": mine["median_ms"], "parent_median_ms": pm, "parent_runs_median_ms": [x["median_ms"] for x in theirs],
                                     "ratio": mine["median_ms"] / pm, "spread_ms": spread, "inside_spread": bool(abs(mine["median_ms"] - pm) <= spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=ROOT, help="the tree whose av_aloha_amd package is measured (default: this one)")
    ap.add_argument("--depth-only", action="store_true", help="avsim_render_depth alone: what a tree without the label image can run")
    ap.add_argument("--parent-json", action="append", default=[], help="a --depth-only result of the parent commit's tree (may be given more than once)")
    ap.add_argument("--add-parent", action="store_true", help="only amend the profile of --tag / --out with --parent-json (needs no GPU)")
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", f"segment_{args.tag}.json")
    parents = []
    for p in args.parent_json:
        with open(p) as f:
            parents.append(json.load(f))
    if args.add_parent:
        with open(path) as f:
            res = json.load(f)
        res["depth_call_against_parent"] = against_parent(res, parents)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["depth_call_against_parent"], indent=1))
        return
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    name = torch.cuda.get_device_name(0)

    def save(r):
        with open(path, "w") as f:
            json.dump({"device": name, "depth_only": args.depth_only, **r}, f, indent=1)

    res = bench(args.envs, args.rounds, args.warmup, args.depth_only, save)
    if parents:
        res["depth_call_against_parent"] = against_parent(res, parents)
    save(res)
    print(json.dumps({k: v for k, v in res.items() if k != "shapes"}, indent=1))


if __name__ == "__main__":
    main()
