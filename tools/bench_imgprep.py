"""What the device's image preparation and image statistics (avsim_image_prep, avsim_image_stats) cost next to the way the tree went before
them.  Writes profiles/imgprep_<tag>.json.

    python tools/bench_imgprep.py --frames 256 --tag r12
    rocprofv3 --kernel-trace --stats -d trace -- python tools/bench_imgprep.py --prep-only 256       # the kernels alone, in a run of its own

The same n JPEG streams (rendered 480 x 640 frames, SlotInsertion, zed_cam_left, quality 90) become normalised float32 CHW crops of
432 x 576 (the centred box), and uncropped images, in two ways; HIP events around the decode and around what follows it, the two ways
alternating in one process, medians over the rounds and the smallest and largest round next to them (the spread a difference has to beat):
  (a) avsim_jpeg_decode to float32 CHW, a torch slice, (x - mean) / std        -- 12 B per pixel written, read, written again
  (b) avsim_jpeg_decode to u8 HWC, avsim_image_prep with imgprep.normalise_lut   -- 3 B per pixel written and read, 12 B written
Both results are compared bit for bit.  k_image_prep's write rate is the bytes of its output over the time of the call, against the 8 TB/s
HBM roof.  The statistics: avsim_image_stats of the u8 batch against torch's float64 sum, sum of squares, amin and amax per image and channel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W = 480, 640
CROP = (432, 576)
HBM_ROOF = 8e12
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def bench(n, rounds, warmup):
    import numpy as np
    import torch
    from av_aloha_amd import imgprep
    from bench_jpeg_decode import decode_call, streams_of
    env, frames, buf, ln = streams_of(n)
    dev = env.device
    f32 = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev)
    u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    mean = torch.tensor(MEAN, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    lut = torch.from_numpy(np.ascontiguousarray(imgprep.normalise_lut(MEAN, STD)).reshape(1, 3, 256)).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    res = {"frames": n, "height": H, "width": W}

    def way_a(oh, ow, x0, y0):
        ev[0].record()
        decode_call(env, buf, ln, 1, 0, f32, status)
        ev[1].record()
        out = (f32[:, :, y0:y0 + oh, x0:x0 + ow] - mean) / std
        ev[2].record()
        torch.cuda.synchronize()
        return out, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    def way_b(oh, ow, box, out):
        ev[0].record()
        decode_call(env, buf, ln, 0, 0, u8, status)
        ev[1].record()
        env.prep_images(u8, lut, box, (oh, ow), out=out)
        ev[2].record()
        torch.cuda.synchronize()
        return out, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])

    for name, (oh, ow) in (("crop_432x576", CROP), ("uncropped", (H, W))):
        x0, y0 = imgprep.center_box((H, W), (oh, ow))
        box = np.tile(np.array([[x0, y0, 0]], dtype=np.int32), (n, 1))
        out_b = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
        t = {k: [] for k in ("a_decode", "a_post", "a_total", "b_decode", "b_post", "b_total")}
        for r in range(warmup + rounds):
            a, ad, ap = way_a(oh, ow, x0, y0)
            b, bd, bp = way_b(oh, ow, box, out_b)
            if r == 0:
                equal = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
            del a
            if r >= warmup:
                for k, v in zip(t, (ad, ap, ad + ap, bd, bp, bd + bp)):
                    t[k].append(v)
        post = statistics.median(t["b_post"])
        res[name] = {"out_h": oh, "out_w": ow, "equal_bits": equal, **{k: summary(v) for k, v in t.items()},
                     "b_over_a_total": statistics.median(t["b_total"]) / statistics.median(t["a_total"]),
                     "a_total_spread": (max(t["a_total"]) - min(t["a_total"])) / statistics.median(t["a_total"]),
                     "prep_bytes_written": n * 3 * oh * ow * 4, "prep_bytes_read": n * 3 * oh * ow,
                     "prep_write_rate_TBps": n * 3 * oh * ow * 4 / (post * 1e-3) / 1e12,
                     "prep_write_rate_over_hbm_roof": n * 3 * oh * ow * 4 / (post * 1e-3) / HBM_ROOF}
    assert not bool(status.any())

    # statistics of the u8 batch
    decode_call(env, buf, ln, 0, 0, u8, status)
    sums = torch.empty((n, 3, 4), dtype=torch.int64, device=dev)
    t = {"avsim_image_stats": [], "torch_float64": []}
    for r in range(warmup + rounds):
        ev[0].record()
        env.image_stats(u8, out=sums)
        ev[1].record()
        x = u8.to(torch.float64)
        ref = (x.sum((1, 2)), (x * x).sum((1, 2)), u8.amin((1, 2)), u8.amax((1, 2)))
        ev[2].record()
        torch.cuda.synchronize()
        if r == 0:
            equal = all(bool(torch.equal(sums[:, :, k], ref[k].to(torch.int64))) for k in range(4))
        del x
        if r >= warmup:
            t["avsim_image_stats"].append(ev[0].elapsed_time(ev[1]))
            t["torch_float64"].append(ev[1].elapsed_time(ev[2]))
    med = statistics.median(t["avsim_image_stats"])
    res["stats"] = {"equal": equal, **{k: summary(v) for k, v in t.items()}, "bytes_read": n * H * W * 3,
                    "read_rate_TBps": n * H * W * 3 / (med * 1e-3) / 1e12,
                    "torch_over_avsim": statistics.median(t["torch_float64"]) / med}
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prep-only", type=int, default=0, help="only decode this many frames to u8 and prepare them ten times (for a kernel trace)")
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_imgprep: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    if args.prep_only:
        import numpy as np
        from av_aloha_amd import imgprep
        from bench_jpeg_decode import decode_call, streams_of
        n = args.prep_only
        env, frames, buf, ln = streams_of(n)
        u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=env.device)
        status = torch.empty(n, dtype=torch.int32, device=env.device)
        lut = torch.from_numpy(np.ascontiguousarray(imgprep.normalise_lut(MEAN, STD)).reshape(1, 3, 256)).to(env.device)
        x0, y0 = imgprep.center_box((H, W), CROP)
        box = np.tile(np.array([[x0, y0, 0]], dtype=np.int32), (n, 1))
        out = torch.empty((n, 3) + CROP, dtype=torch.float32, device=env.device)
        for _ in range(10):
            decode_call(env, buf, ln, 0, 0, u8, status)
            env.prep_images(u8, lut, box, CROP, out=out)
            env.image_stats(u8)
        torch.cuda.synchronize()
        env.close()
        return
    res = {"device": torch.cuda.get_device_name(0), **bench(args.frames, args.rounds, args.warmup)}
    path = args.out or os.path.join(ROOT, "profiles", f"imgprep_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
