"""What per-env observation histories on the device (avsim_obs_history_push) cost next to the same result from torch tensor ops.  Writes
profiles/obshist_<tag>.json.

    python tools/bench_obshist.py --envs 64,256 --steps 2 --crop 432,576 --tag dev

N envs, one camera of --size u8 images (the "gym" format), cropped to --crop and normalised, K = --steps slots, a state of 21 values with
mean / std; a tenth of the envs start an episode in every call (another tenth each call).  Two ways, HIP events around each CALL, two warm-up
rounds, the two ways alternating call by call in one process, medians over nine rounds of `--calls` calls each with the smallest and the
largest round next to them (the spread a difference has to beat):
  (a) VecEnv.prep_images for the new frame, then per slot torch.where(fresh, new, old[k + 1]) -- the shift -- and torch.stack, the state alike;
  (b) obshist.ObsHistory.push: one bookkeeping launch, one state pass, one image pass.
The tool asserts that (a) and (b) are EQUAL, every float of every history, after every call.  Bytes (b) must move per call: the crop's
source bytes, and per env 4 S (2 K - 1) history bytes (S = 3 h w; K - 1 slots read, K written) or 4 S K for a fresh env, the state alike;
(b)'s rate is those bytes over the time of the call, against the 8 TB/s HBM roof."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ROOF = 8e12
PEG = "gym_guided_vision/InsertPeg-3Arms-v0"
CAM = "cam"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


class TorchHistory:
    """av_aloha_amd/obshist.py as tensor ops around VecEnv.prep_images"""

    def __init__(self, env, K, D, lut, box, crop, mean, std):
        torch, dev, N = env.torch, env.device, env.num_envs
        self.env, self.torch, self.K, self.crop = env, torch, K, crop
        self.lut = torch.from_numpy(lut.reshape(1, 3, 256)).to(dev)
        self.box = [tuple(box)] * N
        self.mean, self.std = mean, std
        self.img = torch.zeros((N, K, 3) + tuple(crop), dtype=torch.float32, device=dev)
        self.state = torch.zeros((N, K, D), dtype=torch.float32, device=dev)
        self.last_id = torch.full((N,), -1, dtype=torch.int64, device=dev)

    def _put(self, hist, new, fresh):
        f = fresh.view(-1, *([1] * (new.ndim - 1)))
        return self.torch.stack([self.torch.where(f, new, hist[:, k + 1]) for k in range(self.K - 1)] + [new], dim=1)

    def push(self, state, img, ids, elapsed):
        fresh = (elapsed == 0) | (ids != self.last_id)
        self.state = self._put(self.state, (state - self.mean) / self.std, fresh)
        self.img = self._put(self.img, self.env.prep_images(img, self.lut, self.box, self.crop), fresh)
        self.last_id = ids.clone()
        return self.state, self.img


def bench(N, K, size, crop, calls, rounds, warmup):
    import numpy as np
    import torch
    from av_aloha_amd import imgprep
    from av_aloha_amd import obshist as oh
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(PEG, N, 1000, cameras=[])
    dev, D = env.device, 21
    rng = np.random.default_rng(N)
    stats = {"observation.state": {"mean": rng.standard_normal(D).astype(np.float32), "std": (rng.random(D) + 0.25).astype(np.float32)},
             f"observation.images.{CAM}": {"mean": np.array([0.4, 0.5, 0.6], np.float32), "std": np.array([0.2, 0.25, 0.3], np.float32)}}
    mean, std = (torch.from_numpy(stats["observation.state"][n]).to(dev) for n in ("mean", "std"))
    H, W = size
    src = [torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(4)]
    states = torch.from_numpy(rng.standard_normal((4, N, D)).astype(np.float32)).to(dev)
    total = (warmup + rounds) * calls
    # call t: env e starts an episode when (e + t) % 10 == 0
    e = np.arange(N)
    ids = [torch.from_numpy(e + N * ((e + t) // 10)).to(dev) for t in range(total)]
    elapsed = [torch.from_numpy(((e + t) % 10).astype(np.int32)).to(dev) for t in range(total)]
    nfresh = [N if t == 0 else int(((e + t) % 10 == 0).sum()) for t in range(total)]
    hb = oh.ObsHistory(env, K, stats=stats, crop=crop, cameras=[CAM], state_dim=D, fmt="gym", size=size)
    x0, y0 = imgprep.center_box(size, crop)
    ha = TorchHistory(env, K, D, imgprep.normalise_lut(stats[f"observation.images.{CAM}"]["mean"], stats[f"observation.images.{CAM}"]["std"]).astype(np.float32),
                      (x0, y0, 0), crop, mean, std)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_ms = {"a_torch": [], "b_push": []}
    S = 3 * crop[0] * crop[1]
    moved = []
    for r in range(warmup + rounds):
        per = {"a_torch": [], "b_push": []}
        for c in range(calls):
            t = r * calls + c
            obs = {"observation.state": states[t % 4], f"observation.images.{CAM}": src[t % 4]}
            info = {"episode_id": ids[t], "elapsed_steps": elapsed[t]}
            ev[0].record()
            sa, ia = ha.push(states[t % 4], src[t % 4], ids[t], elapsed[t])
            ev[1].record()
            ev[2].record()
            out = hb.push(obs, info)
            ev[3].record()
            torch.cuda.synchronize()
            per["a_torch"].append(ev[0].elapsed_time(ev[1]))
            per["b_push"].append(ev[2].elapsed_time(ev[3]))
            assert torch.equal(sa, out["observation.state"]) and torch.equal(ia, out[f"observation.images.{CAM}"]), f"call {t}: torch ops and avsim_obs_history_push differ"
            if r >= warmup:
                f = nfresh[t]
                moved.append(N * S + 4 * (S + D) * ((N - f) * (2 * K - 1) + f * K) + 4 * N * D)
        if r >= warmup:
            for key in per:
                t_ms[key].append(statistics.median(per[key]))
    ma, mb = statistics.median(t_ms["a_torch"]), statistics.median(t_ms["b_push"])
    bytes_b = statistics.mean(moved)
    out = {**{key: summary(v) for key, v in t_ms.items()}, "a_over_b": ma / mb,
           "a_spread": (max(t_ms["a_torch"]) - min(t_ms["a_torch"])) / ma, "b_spread": (max(t_ms["b_push"]) - min(t_ms["b_push"])) / mb,
           "b_beats_a_by_more_than_both_spreads": bool(max(t_ms["b_push"]) < min(t_ms["a_torch"])),
           "equal_on_every_call": True, "calls_per_round": calls, "b_bytes_moved": bytes_b, "b_rate_TBps": bytes_b / (mb * 1e-3) / 1e12,
           "b_rate_over_hbm_roof": bytes_b / (mb * 1e-3) / HBM_ROOF}
    print(N, json.dumps(out), flush=True)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,256")
    ap.add_argument("--steps", type=int, default=2, help="n_obs_steps")
    ap.add_argument("--size", default="480,640", help="the source images' height,width")
    ap.add_argument("--crop", default="432,576")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_obshist: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    size, crop = (tuple(int(v) for v in s.split(",")) for s in (args.size, args.crop))
    res = {"device": torch.cuda.get_device_name(0), "n_obs_steps": args.steps, "size": size, "crop": crop, "format": "gym (u8 HWC)", "envs": {}}
    for n in (int(v) for v in args.envs.split(",")):
        res["envs"][str(n)] = bench(n, args.steps, size, crop, args.calls, args.rounds, args.warmup)
    path = args.out or os.path.join(ROOT, "profiles", f"obshist_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
