"""What the device's virtual orthographic views (avsim_virtual_views) cost next to the same result as torch tensor ops.  Writes
profiles/virtviews_<tag>.json.

    python tools/bench_virtviews.py --tag r20

256 and 1024 envs of slot_insertion at their reset poses, three cameras (the ZED left camera and the two wrist cameras) at 84 x 112, the
depth and the u8 colour images rendered once, the workspace box BOUNDS, the five views +z +x -x +y -y at 110 x 110 and 220 x 220, radius 0
and 1, with and without colour; HIP events around each way, the ways alternating in one process after warm-up -- in an order that rotates by
one from round to round, and with (b) and (c) writing the same output buffers --, medians over the rounds and the smallest and largest round
next to them (the spread a difference has to beat):
  (a) torch on the GPU from the same depth, colour and pose tensors: the specification's formulas as tensor ops -- deprojection, mask, pixel
      coordinates, int64 keys (the dist's bits above the slot) --, one scatter_reduce_("amin") per view and footprint offset into a buffer of
      keys, then gathers of the winners' points and colours.  A pixel that is no candidate scatters the empty key, so nothing is compacted
      and nothing synchronises
  (b) avsim_virtual_views as the library was built: the pose kernel, clear, scatter, finish
  (c) the same call with each of the four scatter forms named outright (option "virtviews_form" f + 1: bit 0 of f the load before the
      atomic, bit 1 the merge of runs in the wave); what ships is one of them, or a choice among them per call (the build's AVSIM_VV_FORM)
      -- the tool does not know which and does not need to
Conditions (asserted at the end, after the profile is written): the median of (b) is below the fastest round of (a) in every case, and (b)
is not slower than any form of (c) beyond the two's own round-to-round spread.  (b) and every (c) give the same bytes (a minimum; asserted).
Whether (a)'s index equals (b)'s is reported, not asserted.  With each case: the bytes the three passes move and the time they would take at
the HBM roof (6.29 TB/s measured copy rate of the part, 8 TB/s nominal), and the atomic wave-instructions and lane atomics the scatter
issues at most -- without the load, which skips a number of them that depends on the order of arrival; with and without the merge --, all
computed from the candidates' pixels with tensor ops, in the kernel's own assignment of pixels to waves (256 consecutive pixels of an env
per workgroup)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMS = ["zed_cam_left", "wrist_cam_left", "wrist_cam_right"]
H, W = 84, 112
BOUNDS = (-0.6, -0.5, -0.05, 0.6, 0.7, 0.8)
VIEWS = ["+z", "+x", "-x", "+y", "-y"]
SIZES = [110, 220]
RADII = [0, 1]
FORMS = {0: "plain", 1: "load", 2: "merge", 3: "load_and_merge"}
HBM_MEASURED, HBM_NOMINAL = 6.29e12, 8.0e12
# per code: (dist axis, dist from hi, column axis, column descending, row axis, row descending) -- virtviews.VIEW_AXES
EMPTY = (1 << 63) - 1          # way (a)'s empty key: int64's largest (a dist is >= 0, so every real key is below it)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


def torch_points(torch, poses, depth, lo, hi, max_depth):
    """(world float32 [N, Q, 3], mask [N, Q]) with plain tensor ops: the specification's deprojection and candidate rule."""
    N, C, Hh, Ww = depth.shape
    dev = depth.device
    pc_, R, t = poses[:, :, :3], poses[:, :, 3:12].reshape(N, C, 3, 3), poses[:, :, 12]
    scale = (2.0 * t / float(Hh)).reshape(N, C, 1, 1)
    x = ((torch.arange(Ww, dtype=torch.float32, device=dev) + 0.5) - 0.5 * Ww).reshape(1, 1, 1, Ww) * scale
    y = -(((torch.arange(Hh, dtype=torch.float32, device=dev) + 0.5) - 0.5 * Hh).reshape(1, 1, Hh, 1) * scale)
    X, Y, Z = x * depth, y * depth, -depth
    w = torch.stack([((pc_[:, :, i, None, None] + R[:, :, i, 0, None, None] * X) + R[:, :, i, 1, None, None] * Y) + R[:, :, i, 2, None, None] * Z for i in range(3)], dim=-1)
    w = w.reshape(N, C * Hh * Ww, 3)
    return w, (depth.reshape(N, -1) < max_depth) & ((w >= lo) & (w <= hi)).all(dim=-1)


def torch_pixels(torch, w, lo, hi, k, n, descending):
    """int64 [N, Q]: the pixel of coordinate k on an image axis of n (clamped: a pixel outside the box names one too)."""
    u = (w[:, :, k] - lo[k]) * (float(n) / (hi[k] - lo[k]))
    i = torch.floor(u).nan_to_num_(nan=0.0).clamp_(0.0, float(n - 1)).to(torch.int64)
    return (n - 1 - i) if descending else i


def torch_targets(torch, w, lo, hi, codes, size):
    """Per view (dist float32 [N, Q], row int64 [N, Q], column int64 [N, Q])."""
    from av_aloha_amd.virtviews import VIEW_AXES
    res = []
    for code in codes:
        da, from_hi, ca, cdesc, ra, rdesc = VIEW_AXES[code]
        dist = (hi[da] - w[:, :, da]) if from_hi else (w[:, :, da] - lo[da])
        res.append((dist, torch_pixels(torch, w, lo, hi, ra, size, rdesc), torch_pixels(torch, w, lo, hi, ca, size, cdesc)))
    return res


def torch_views(torch, poses, depth, rgb, lo, hi, max_depth, codes, size, radius):
    """Way (a): (out float32 [N, V, S, S, 8], index int32 [N, V, S, S])."""
    N, Q = depth.shape[0], depth.shape[1] * depth.shape[2] * depth.shape[3]
    dev, V, P = depth.device, len(codes), size * size
    w, mask = torch_points(torch, poses, depth, lo, hi, max_depth)
    empty = torch.full((), EMPTY, dtype=torch.int64, device=dev)
    keys = torch.full((N * V * P,), EMPTY, dtype=torch.int64, device=dev)
    slot = torch.arange(Q, dtype=torch.int64, device=dev)[None, :]
    base = torch.arange(N, dtype=torch.int64, device=dev)[:, None] * (V * P)
    for v, (dist, pr, pc_) in enumerate(torch_targets(torch, w, lo, hi, codes, size)):
        key = torch.where(mask, (dist.contiguous().view(torch.int32).to(torch.int64) << 32) | slot, empty)
        for dr in range(-radius, radius + 1):
            for dc in range(-radius, radius + 1):
                r, c = pr + dr, pc_ + dc
                inside = (r >= 0) & (r < size) & (c >= 0) & (c < size)
                idx = base + v * P + r.clamp(0, size - 1) * size + c.clamp(0, size - 1)
                keys.scatter_reduce_(0, idx.reshape(-1), torch.where(inside, key, empty).reshape(-1), "amin")
    keys = keys.reshape(N, V * P)
    hit = keys != EMPTY
    win = torch.where(hit, keys & 0xFFFFFFFF, torch.zeros_like(keys))
    out = torch.zeros((N, V * P, 8), dtype=torch.float32, device=dev)
    hf = hit.to(torch.float32)
    if rgb is not None:
        out[:, :, 0:3] = torch.gather(rgb.reshape(N, Q, 3), 1, win[:, :, None].expand(-1, -1, 3)).to(torch.float32) * (1.0 / 255.0) * hf[:, :, None]
    out[:, :, 3] = torch.where(hit, (keys >> 32).to(torch.int32).view(torch.float32), torch.zeros_like(hf))
    out[:, :, 4:7] = torch.where(hit[:, :, None], torch.gather(w, 1, win[:, :, None].expand(-1, -1, 3)), torch.zeros_like(out[:, :, 4:7]))
    out[:, :, 7] = hf
    index = torch.where(hit, win, torch.full_like(win, -1)).to(torch.int32)
    return out.reshape(N, V, size, size, 8), index.reshape(N, V, size, size)


def scatter_statistics(torch, mask, targets, size, radius):
    """The scatter pass in numbers, from the candidates' pixels in the kernel's own lanes: 256 consecutive pixels of an env per workgroup."""
    N, Q = mask.shape
    pad = (-Q) % 256
    cand, waves = int(mask.sum()), 0
    wave_instr = lanes_plain = lanes_merged = runs_total = 0
    for dist, pr, pc_ in targets:
        tgt = torch.where(mask, pr * size + pc_, torch.full_like(pr, -1))
        if pad:
            tgt = torch.cat([tgt, torch.full((N, pad), -1, dtype=tgt.dtype, device=tgt.device)], dim=1)
        r = torch.nn.functional.pad(pr, (0, pad)).reshape(N, -1, 64)
        c = torch.nn.functional.pad(pc_, (0, pad)).reshape(N, -1, 64)
        tgt = tgt.reshape(N, -1, 64)
        valid = tgt >= 0
        head = torch.ones_like(valid)
        head[:, :, 1:] = tgt[:, :, 1:] != tgt[:, :, :-1]
        head &= valid
        # the pixels of a lane's footprint that lie inside the image
        fp = ((torch.minimum(r + radius, torch.full_like(r, size - 1)) - (r - radius).clamp(min=0) + 1) * (torch.minimum(c + radius, torch.full_like(c, size - 1)) - (c - radius).clamp(min=0) + 1))
        waves = int(valid.any(dim=2).sum())
        # a wave issues as many atomic instructions per view as its busiest lane has pixels
        wave_instr += int(torch.where(valid, fp, torch.zeros_like(fp)).amax(dim=2).sum())
        lanes_plain += int(torch.where(valid, fp, torch.zeros_like(fp)).sum())
        lanes_merged += int(torch.where(head, fp, torch.zeros_like(fp)).sum())
        runs_total += int(head.sum())
    V = len(targets)
    return {"candidates": cand, "waves_with_candidates": waves, "runs": runs_total, "mean_run_length": cand * V / max(runs_total, 1),
            "atomic_wave_instructions_at_most": wave_instr, "lane_atomics_at_most_plain": lanes_plain, "lane_atomics_at_most_merged": lanes_merged}


def bench(envs, rounds, warmup, save):
    import numpy as np
    import torch
    from av_aloha_amd import pointcloud, virtviews
    from av_aloha_amd.vec_env import VecEnv
    codes = list(virtviews.view_codes(VIEWS))
    res = {"cameras": CAMS, "height": H, "width": W, "bounds": list(BOUNDS), "views": VIEWS, "forms": FORMS, "cases": {}}
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
        w, mask = torch_points(torch, poses, depth, lo, hi, pointcloud.FAR_PLANE)

        def form(f):
            env.h.check(env.L.avsim_set_option(env.h.h, b"virtviews_form", float(f)))

        for size in SIZES:
            targets = torch_targets(torch, w, lo, hi, codes, size)
            for radius in RADII:
                stats = scatter_statistics(torch, mask, targets, size, radius)
                for colour in (False, True):
                    rgb = rgb8 if colour else None
                    # (b) and every (c) write the SAME two buffers: the same kernel on two allocations of this size differs by more than the forms do
                    buf = (torch.empty((N, len(codes), size, size, 8), dtype=torch.float32, device=dev), torch.empty((N, len(codes), size, size), dtype=torch.int32, device=dev))

                    def way_a():
                        return torch_views(torch, poses, depth, rgb, lo, hi, pointcloud.FAR_PLANE, codes, size, radius)

                    def call(f):
                        def run():
                            form(f)
                            r = env.virtual_views(CAMS, H, W, bounds, codes, size, radius=radius, depth=depth, rgb=rgb, out=buf[0], index=buf[1])
                            form(0)
                            return r
                        return run

                    ways = [("a_torch", way_a), ("b_shipped", call(0))] + [(f"c_{name}", call(f + 1)) for f, name in FORMS.items()]
                    b = tuple(x.clone() for x in ways[1][1]())
                    for k, way in ways[2:]:
                        o, i = way()
                        assert torch.equal(o.view(torch.int32), b[0].view(torch.int32)) and torch.equal(i, b[1]), f"scatter form {k} differs from the shipped one"
                    a = way_a()
                    torch.cuda.synchronize()
                    a_index_equal = bool(torch.equal(a[1], b[1]))
                    a_index_differs = int((a[1] != b[1]).sum())
                    a_out_equal = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
                    hits = int((b[1] >= 0).sum())
                    del a, b
                    t = {k: [] for k, _ in ways}
                    for r in range(warmup + rounds):
                        for key, way in ways[r % len(ways):] + ways[:r % len(ways)]:          # (rotated: every way follows every other one equally often)
                            ev[0].record()
                            y = way()
                            ev[1].record()
                            torch.cuda.synchronize()
                            del y
                            if r >= warmup:
                                t[key].append(ev[0].elapsed_time(ev[1]))
                    med = {k: statistics.median(v) for k, v in t.items()}
                    spread = {k: max(v) - min(v) for k, v in t.items()}
                    vpix = N * len(codes) * size * size
                    Q = N * len(CAMS) * H * W
                    moved = {"clear_write": 16 * vpix, "scatter_read_depth": 4 * Q, "scatter_atomics_at_most_plain": 8 * stats["lane_atomics_at_most_plain"],
                             "finish_read_keys": 8 * vpix, "finish_read_winners": hits * (7 if colour else 4), "finish_write": 36 * vpix}
                    total = sum(moved.values())
                    c_keys = [k for k in t if k.startswith("c_")]
                    worst = max(c_keys, key=lambda k: (med["b_shipped"] - med[k]) - max(spread["b_shipped"], spread[k]))
                    key = f"{N}_envs_size{size}_radius{radius}_{'colour' if colour else 'depth_only'}"
                    res["cases"][key] = {**{k: summary(v) for k, v in t.items()}, "envs": N, "size": size, "radius": radius, "colour": colour, "pixels": Q, "virtual_pixels": vpix,
                                         "hit_virtual_pixels": hits, "a_min_over_b_median": min(t["a_torch"]) / med["b_shipped"],
                                         "b_median_below_a_min": bool(med["b_shipped"] < min(t["a_torch"])),
                                         "b_minus_c_median_ms": {k: med["b_shipped"] - med[k] for k in c_keys},
                                         "b_c_spread_ms": {k: max(spread["b_shipped"], spread[k]) for k in c_keys},
                                         "b_not_slower_than_c_beyond_spread": bool(med["b_shipped"] - med[worst] <= max(spread["b_shipped"], spread[worst])),
                                         "fastest_form_by_median": min(c_keys, key=lambda k: med[k]),
                                         "bytes": {**moved, "total": total}, "ms_at_hbm_measured_6.29TBps": 1e3 * total / HBM_MEASURED, "ms_at_hbm_nominal_8TBps": 1e3 * total / HBM_NOMINAL,
                                         "share_of_hbm_measured_roof": (1e3 * total / HBM_MEASURED) / med["b_shipped"], "scatter": stats,
                                         "index_equals_torch": a_index_equal, "index_differs_from_torch_virtual_pixels": a_index_differs, "out_equals_torch": a_out_equal}
                    print(key, json.dumps(res["cases"][key]), flush=True)
                    save(res)          # (after every case: a run that is cut short leaves what it measured)
                    del buf
        env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    path = args.out or os.path.join(ROOT, "profiles", f"virtviews_{args.tag}.json")
    if args.rounds < 20:
        raise SystemExit("bench_virtviews: at least 20 rounds")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_virtviews: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    name = torch.cuda.get_device_name(0)

    def save(r):
        with open(path, "w") as f:
            json.dump({"device": name, **r}, f, indent=1)

    res = {"device": name, **bench(args.envs, args.rounds, args.warmup, save)}
    save({k: v for k, v in res.items() if k != "device"})
    bad = [k for k, c in res["cases"].items() if not (c["b_median_below_a_min"] and c["b_not_slower_than_c_beyond_spread"])]
    if bad:
        raise SystemExit(f"bench_virtviews: the conditions do not hold in {bad}")
    print("bench_virtviews: the conditions hold in all", len(res["cases"]), "cases")


if __name__ == "__main__":
    main()
