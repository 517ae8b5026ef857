"""What the device's colour, sharpness and affine augmentation (avsim_image_jitter, avsim_image_augment) costs next to the same arithmetic as torch tensor ops.  Writes
profiles/imgaug_<tag>.json.

    python tools/bench_imgaug.py --frames 256 --tag r13

n decoded 480 x 640 u8 frames (rendered, SlotInsertion, zed_cam_left, through the JPEG encoder and decoder at quality 90) become normalised
float32 CHW crops of 432 x 576 (random boxes, no mirror) in two ways; HIP events around each, the two ways alternating in one process,
medians over the rounds and the smallest and largest round next to them (the spread a difference has to beat):
  (a) avsim_image_prep with imgprep.identity_lut (the crop in [0, 1]), then brightness, contrast, saturation, hue and sharpness as torch
      tensor ops on the whole batch -- the formulas of av_aloha_amd/imgaug.py, an op an image does not have selected away by torch.where --
      and (x - mean) / std: every op a read and a write of n x 3 x 432 x 576 floats or several
  (b) avsim_image_jitter: the u8 frames read once (once more, whole, by the reduction for the images that have contrast), the floats written once
Cases: every single op on all images, LeRobot's default plan (imgaug.augment_plan: 3 of 5 per image) and all five.  (a) works on the crop:
its contrast mean is the crop's and its blur stops at the crop's border, where (b)'s are the source image's; torch's reductions and its
convolution also round in their own order.  So the largest absolute difference between the two (before the normalisation, over all pixels
and over those not on the crop's border) is reported, not asserted -- tests/test_gpu_imgaug.py compares (b) with the specification for
equality.  Bytes: (b) writes 12 B and reads 3 B per output pixel, and 3 B per source pixel of every image that has contrast; its rate is
those bytes over the time of the call, against the 8 TB/s HBM roof.

The geometric op (avsim_image_augment), cases "affine" (bit 5 on all images, nearest), "affine_bilinear", "default+affine"
(imgaug.LEROBOT_CFG's plan: 3 of 6 per image, nearest) and "sharpness+affine" (mask 48 on all images, nearest).  The op runs on the whole
frame before the crop, so way (a) cannot start from the crop: it is u8 -> float32 CHW of the whole frames, the colour formulas on them,
F.affine_grid + F.grid_sample(padding_mode="zeros", align_corners=False) with the same matrices (images without the bit get the identity),
one gather for the boxes, (x - mean) / std; way (b) is the one call.  The two differ where a source coordinate rounds the other way
(nearest) and by rounding (bilinear), so the largest difference and the share of values that differ by more than 1e-3 are reported.
Bytes of (b), counted as what has to move, not what the caches saw: 12 B written per output value triple; read 3 B per output pixel (its
taps lie next to its neighbours' -- bilinear's four are the same lines), 3 B per source pixel of an image that has contrast; an image
with sharpness and bit 5 also reads its whole frame (3 B per pixel), writes and reads it as floats once (12 B per pixel written, 12 B per
output pixel read back)."""
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


def torch_ops(torch):
    """The five formulas on float32 [n, 3, h, w] in [0, 1]; f: [n, 1, 1, 1]."""
    def blend(a, b, f):
        return (a * f + b * (1 - f)).clamp(0, 1)

    def gray(x):
        return (0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2]) + 0.114 * x[:, 2:3]

    def brightness(x, f):
        return (x * f).clamp(0, 1)

    def contrast(x, f):
        return blend(x, gray(x).mean(dim=(1, 2, 3), keepdim=True), f)

    def saturation(x, f):
        return blend(x, gray(x), f)

    def hue(x, f):
        r, g, b = x[:, 0], x[:, 1], x[:, 2]
        f = f[:, 0]
        maxc, minc = x.amax(dim=1), x.amin(dim=1)
        eqc = maxc == minc
        cr = maxc - minc
        ones = torch.ones_like(maxc)
        s = cr / torch.where(eqc, ones, maxc)
        crd = torch.where(eqc, ones, cr)
        rc, gc, bc = (maxc - r) / crd, (maxc - g) / crd, (maxc - b) / crd
        h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
        h = h / 6.0 + 1.0
        h = h - h.floor()
        h = h + f
        h = h - h.floor()
        h6 = h * 6.0
        fl = h6.floor()
        ff = h6 - fl
        i = fl.to(torch.int32) % 6
        v = maxc
        p = (v * (1 - s)).clamp(0, 1)
        q = (v * (1 - s * ff)).clamp(0, 1)
        t = (v * (1 - s * (1 - ff))).clamp(0, 1)

        def six(a):
            out = a[5]
            for k in (4, 3, 2, 1, 0):
                out = torch.where(i == k, a[k], out)
            return out

        return torch.stack([six((v, q, p, p, t, v)), six((t, v, v, q, p, p)), six((p, p, t, v, v, q))], dim=1)

    kernel = torch.ones((1, 1, 3, 3)) / 13
    kernel[0, 0, 1, 1] = 5 / 13

    def sharpness(x, f):
        n, c, h, w = x.shape
        blur = torch.nn.functional.conv2d(x.reshape(n * c, 1, h, w), kernel.to(x.device)).reshape(n, c, h - 2, w - 2)
        out = x.clone()
        out[:, :, 1:-1, 1:-1] = blend(x[:, :, 1:-1, 1:-1], blur, f)
        return out

    return [brightness, contrast, saturation, hue, sharpness]


def bench(n, rounds, warmup):
    import numpy as np
    import torch
    from av_aloha_amd import imgaug, imgprep
    from bench_jpeg_decode import decode_call, streams_of
    env, frames, buf, ln = streams_of(n)
    dev = env.device
    u8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    decode_call(env, buf, ln, 0, 0, u8, status)
    torch.cuda.synchronize()
    assert not bool(status.any())
    del frames, buf
    oh, ow = CROP
    mean = torch.tensor(MEAN, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1)
    lut = torch.from_numpy(np.ascontiguousarray(imgprep.identity_lut()).reshape(1, 3, 256)).to(dev)
    rng = np.random.default_rng(0)
    box = np.zeros((n, 3), dtype=np.int32)
    box[:, 1], box[:, 0] = rng.integers(0, H - oh + 1, n), rng.integers(0, W - ow + 1, n)
    ops = torch_ops(torch)
    crop01 = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
    out_b = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"frames": n, "height": H, "width": W, "out_h": oh, "out_w": ow, "cases": {}}

    plan = imgaug.augment_plan(n, None, seed=0)
    cases = [(name, np.full(n, 1 << k, dtype=np.int32)) for k, name in enumerate(imgaug.OPS)] + [("default_plan_3_of_5", plan[0]), ("all_five", np.full(n, 31, dtype=np.int32))]
    for name, mask in cases:
        if name == "default_plan_3_of_5":
            fac = plan[1]
        else:
            fac = np.stack([rng.uniform(*imgaug.DEFAULT_CFG[op]["min_max"], n) for op in imgaug.OPS], axis=1).astype(np.float32)
        params = imgaug.pack_params(box, mask, fac)
        t_fac = [torch.from_numpy(np.ascontiguousarray(fac[:, k])).to(dev).reshape(n, 1, 1, 1) for k in range(5)]
        t_on = [torch.from_numpy(np.ascontiguousarray((mask >> k & 1).astype(bool))).to(dev).reshape(n, 1, 1, 1) for k in range(5)]
        every = [bool((mask >> k & 1).all()) for k in range(5)]
        some = [bool((mask >> k & 1).any()) for k in range(5)]

        def way_a(normalise=True):
            env.prep_images(u8, lut, box, (oh, ow), out=crop01)
            x = crop01
            for k in range(5):
                if some[k]:
                    y = ops[k](x, t_fac[k])
                    x = y if every[k] else torch.where(t_on[k], y, x)
            return (x - mean) / std if normalise else x

        def way_b(normalise=True):
            return env.jitter_images(u8, params, (oh, ow), MEAN if normalise else None, STD if normalise else None, out=out_b)

        # the difference of the two ways, in [0, 1]
        a, b = way_a(False), way_b(False)
        torch.cuda.synchronize()
        d = (a - b).abs()
        diff, diff_inside = float(d.max()), float(d[:, :, 1:-1, 1:-1].max())
        del a, d
        t = {"a_torch": [], "b_jitter": []}
        for r in range(warmup + rounds):
            for key, way in (("a_torch", way_a), ("b_jitter", way_b)):
                ev[0].record()
                y = way()
                ev[1].record()
                torch.cuda.synchronize()
                del y
                if r >= warmup:
                    t[key].append(ev[0].elapsed_time(ev[1]))
        med = statistics.median(t["b_jitter"])
        ncon = int((mask >> 1 & 1).sum())
        written, read = n * 3 * oh * ow * 4, n * 3 * oh * ow + ncon * 3 * H * W
        res["cases"][name] = {**{k: summary(v) for k, v in t.items()}, "a_over_b": statistics.median(t["a_torch"]) / med,
                              "a_spread": (max(t["a_torch"]) - min(t["a_torch"])) / statistics.median(t["a_torch"]),
                              "images_with_contrast": ncon, "b_bytes_written": written, "b_bytes_read": read,
                              "b_rate_TBps": (written + read) / (med * 1e-3) / 1e12, "b_rate_over_hbm_roof": (written + read) / (med * 1e-3) / HBM_ROOF,
                              "max_abs_diff_0_1": diff, "max_abs_diff_0_1_off_the_crop_border": diff_inside}
        print(name, json.dumps(res["cases"][name]), flush=True)
    bench_affine(env, u8, box, ops, mean, std, out_b, ev, res, rng, warmup, rounds)
    env.close()
    return res


def bench_affine(env, u8, box, ops, mean, std, out_b, ev, res, rng, warmup, rounds):
    """The cases with the geometric op (module docstring)."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from av_aloha_amd import imgaug
    n, dev = int(u8.shape[0]), u8.device
    oh, ow = CROP
    lerobot = imgaug.augment_plan_affine(n, imgaug.LEROBOT_CFG, seed=0, size=(H, W))
    every = imgaug.augment_plan_affine(n, dict(imgaug.LEROBOT_CFG, max_num_transforms=6), seed=1, size=(H, W))      # a matrix for every image
    cases = [("affine", np.full(n, 32, dtype=np.int32), every[1], every[2], 0), ("affine_bilinear", np.full(n, 32, dtype=np.int32), every[1], every[2], 1),
             ("default+affine", lerobot[0], lerobot[1], lerobot[2], 0), ("sharpness+affine", np.full(n, 48, dtype=np.int32), every[1], every[2], 0)]
    iy = torch.from_numpy(box[:, 1, None] + np.arange(oh)[None, :]).to(dev)[:, None, :, None]
    ix = torch.from_numpy(box[:, 0, None] + np.arange(ow)[None, :]).to(dev)[:, None, None, :]
    ii, ic = torch.arange(n, device=dev)[:, None, None, None], torch.arange(3, device=dev)[None, :, None, None]
    for name, mask, fac, mat, interp in cases:
        params = imgaug.pack_params(box, mask, fac)
        t_fac = [torch.from_numpy(np.ascontiguousarray(fac[:, k])).to(dev).reshape(n, 1, 1, 1) for k in range(5)]
        t_on = [torch.from_numpy(np.ascontiguousarray((mask >> k & 1).astype(bool))).to(dev).reshape(n, 1, 1, 1) for k in range(5)]
        all_on = [bool((mask >> k & 1).all()) for k in range(5)]
        some = [bool((mask >> k & 1).any()) for k in range(5)]
        m = np.where((mask & 32).astype(bool)[:, None], mat, imgaug.IDENTITY_MATRIX).astype(np.float64)
        theta = np.stack([np.stack([m[:, 0], m[:, 1] * H / W, m[:, 2] * 2 / W], axis=1), np.stack([m[:, 3] * W / H, m[:, 4], m[:, 5] * 2 / H], axis=1)], axis=1)
        t_theta = torch.from_numpy(theta.astype(np.float32)).to(dev)

        def way_a(normalise=True):
            x = u8.permute(0, 3, 1, 2).to(torch.float32) / 255.0
            for k in range(5):
                if some[k]:
                    y = ops[k](x, t_fac[k])
                    x = y if all_on[k] else torch.where(t_on[k], y, x)
            grid = F.affine_grid(t_theta, (n, 3, H, W), align_corners=False)
            x = F.grid_sample(x, grid, mode="bilinear" if interp else "nearest", padding_mode="zeros", align_corners=False)
            x = x[ii, ic, iy, ix]
            return (x - mean) / std if normalise else x

        def way_b(normalise=True):
            return env.augment_images(u8, params, mat, (oh, ow), interp, MEAN if normalise else None, STD if normalise else None, out=out_b)

        a, b = way_a(False), way_b(False)
        torch.cuda.synchronize()
        d = (a - b).abs()
        diff, share = float(d.max()), float((d > 1e-3).float().mean())
        del a, d
        t = {"a_torch": [], "b_augment": []}
        for r in range(warmup + rounds):
            for key, way in (("a_torch", way_a), ("b_augment", way_b)):
                ev[0].record()
                y = way()
                ev[1].record()
                torch.cuda.synchronize()
                del y
                if r >= warmup:
                    t[key].append(ev[0].elapsed_time(ev[1]))
        med = statistics.median(t["b_augment"])
        ncon, nboth = int((mask >> 1 & 1).sum()), int(((mask & 48) == 48).sum())
        written = n * 3 * oh * ow * 4 + nboth * 12 * H * W
        read = n * 3 * oh * ow + ncon * 3 * H * W + nboth * (3 * H * W + 12 * oh * ow - 3 * oh * ow)
        res["cases"][name] = {**{k: summary(v) for k, v in t.items()}, "a_over_b": statistics.median(t["a_torch"]) / med,
                              "a_spread": (max(t["a_torch"]) - min(t["a_torch"])) / statistics.median(t["a_torch"]), "interp": interp,
                              "images_with_affine": int((mask >> 5 & 1).sum()), "images_with_contrast": ncon, "images_with_sharpness_and_affine": nboth,
                              "b_bytes_written": written, "b_bytes_read": read,
                              "b_rate_TBps": (written + read) / (med * 1e-3) / 1e12, "b_rate_over_hbm_roof": (written + read) / (med * 1e-3) / HBM_ROOF,
                              "max_abs_diff_0_1": diff, "share_of_values_differing_by_more_than_1e-3": share}
        print(name, json.dumps(res["cases"][name]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_imgaug: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), **bench(args.frames, args.rounds, args.warmup)}
    path = args.out or os.path.join(ROOT, "profiles", f"imgaug_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
