"""What the device's image resize (avsim_image_resize) costs next to the same result as torch tensor ops.  Writes profiles/imgresize_<tag>.json.

    python tools/bench_imgresize.py --tag r17

n = 64 and 256 frames of 480 x 640 u8 (noise from a seed: the kernels do no data-dependent work, and noise is the hardest input for the
difference below) become normalised float32 CHW images in two ways, for two targets -- 224 x 224 letterboxed (imgresize.resize_with_pad_plan:
168 x 224 under 56 rows of zeros) and 96 x 96 stretched -- with antialias on and off; HIP events around each way, the two ways alternating
in one process after warm-up, medians over the rounds and the smallest and largest round next to them (the spread a difference has to beat):
  (a) torch on the GPU from the u8 tensor: permute + float + / 255, F.interpolate(mode="bilinear", align_corners=False, antialias=...),
      F.pad, (x - mean) / std: a float32 copy of the whole frames and several of the output
  (b) avsim_image_resize: the u8 frames read once, the floats written once
The two round differently (torch's antialias kernel keeps its own weight tables and sums; its plain bilinear computes the two weights from
the source index, not from the triangle), so the largest absolute difference between them in [0, 1], before the normalisation, is reported,
not asserted -- tests/test_gpu_imgresize.py compares (b) with the specification for equality, tests/test_imgresize_host.py the specification
with torch's CPU result.  Bytes of (b), counted as what has to move: 3 B read per source pixel (without antialias only the rows and the
32-byte sectors that hold taps are needed; the figure counts whole frames all the same) and 12 B written per output pixel; the rate is those
bytes over the time of the call, against the 8 TB/s HBM roof.  Times are call times from device events; they include the staging copy and
the launch.

--abba-log FILE adds what bench.py gave alternating with the parent's build: the lines "new <env-steps/s> ..." / "old <env-steps/s> ..." that
tools/exp_abba.sh prints (the parent's tree built next to this one), and whether this build's values lie inside the parent's own range
widened by its spread.  With --add-abba the profile of --tag (or --out) is only amended; that needs no GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
HBM_ROOF = 8e12
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TARGETS = [("224x224_letterbox", (224, 224), "pad"), ("96x96_stretch", (96, 96), "stretch")]


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def bench(frames, rounds, warmup):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from av_aloha_amd import imgresize
    from av_aloha_amd.images import DeviceImages
    di = DeviceImages()
    dev = di.device
    mean = torch.tensor(MEAN, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"height": H, "width": W, "cases": {}}
    for n in frames:
        gen = torch.Generator(device=dev)
        gen.manual_seed(n)
        u8 = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
        for name, (oh, ow), mode in TARGETS:
            sb, dst = imgresize.boxes(np.zeros((n, 3), dtype=np.int32), (H, W), (oh, ow), mode)
            ox, oy, rw, rh = (int(v) for v in dst[0])
            out_b = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
            for antialias in (True, False):
                def way_a(normalise=True):
                    x = u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
                    x = F.interpolate(x, size=(rh, rw), mode="bilinear", align_corners=False, antialias=antialias)
                    x = F.pad(x, (ox, ow - rw - ox, oy, oh - rh - oy))
                    return (x - mean) / std if normalise else x

                def way_b(normalise=True):
                    return di.resize_images(u8, sb, dst, (oh, ow), antialias, None, MEAN if normalise else None, STD if normalise else None, out=out_b)

                a, b = way_a(False), way_b(False)
                torch.cuda.synchronize()
                diff = float((a - b).abs().max())
                del a
                t = {"a_torch": [], "b_resize": []}
                for r in range(warmup + rounds):
                    for key, way in (("a_torch", way_a), ("b_resize", way_b)):
                        ev[0].record()
                        y = way()
                        ev[1].record()
                        torch.cuda.synchronize()
                        del y
                        if r >= warmup:
                            t[key].append(ev[0].elapsed_time(ev[1]))
                med = statistics.median(t["b_resize"])
                read, written = n * 3 * H * W, n * 3 * oh * ow * 4
                key = f"{n}_frames_{name}_{'antialias' if antialias else 'plain'}"
                res["cases"][key] = {**{k: summary(v) for k, v in t.items()}, "frames": n, "out_h": oh, "out_w": ow, "dst": [ox, oy, rw, rh], "antialias": antialias,
                                     "a_over_b": statistics.median(t["a_torch"]) / med,
                                     "a_spread": (max(t["a_torch"]) - min(t["a_torch"])) / statistics.median(t["a_torch"]),
                                     "b_spread": (max(t["b_resize"]) - min(t["b_resize"])) / med,
                                     "b_bytes_read": read, "b_bytes_written": written, "b_rate_TBps": (read + written) / (med * 1e-3) / 1e12,
                                     "b_rate_over_hbm_roof": (read + written) / (med * 1e-3) / HBM_ROOF, "max_abs_diff_from_torch_gpu_0_1": diff}
                print(key, json.dumps(res["cases"][key]), flush=True)
        del u8
    di.close()
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
        raise SystemExit(f"bench_imgresize: {path} holds no 'new' / 'old' lines")
    lo, hi = min(runs["old"]), max(runs["old"])
    return {"command": "bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-extras", "unit": "env-steps/s", **runs, "parent_spread": (hi - lo) / statistics.median(runs["old"]),
            "new_median_over_old_median": statistics.median(runs["new"]) / statistics.median(runs["old"]),
            "new_inside_parent_range_widened_by_its_spread": bool(lo - (hi - lo) <= min(runs["new"]) and max(runs["new"]) <= hi + (hi - lo))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    ap.add_argument("--abba-log", default=None)
    ap.add_argument("--add-abba", action="store_true")
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", f"imgresize_{args.tag}.json")
    if args.add_abba:
        with open(path) as f:
            res = json.load(f)
        res["bench_py_alternating_with_parent"] = abba(args.abba_log)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["bench_py_alternating_with_parent"], indent=1))
        return
    if args.rounds < 20:
        raise SystemExit("bench_imgresize: at least 20 rounds")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_imgresize: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), **bench(args.frames, args.rounds, args.warmup)}
    if args.abba_log:
        res["bench_py_alternating_with_parent"] = abba(args.abba_log)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
