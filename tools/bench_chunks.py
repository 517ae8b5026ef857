"""What per-env chunk execution on the device (avsim_chunk_step) costs next to the same formula as torch tensor ops.  Writes
profiles/chunks_<tag>.json.

    python tools/bench_chunks.py --envs 64,1024,4096 --chunk 100 --dim 21 --tag r14

N envs, chunks float32 [N, C, A], both modes of av_aloha_amd/chunks.py with mean / std; a tenth of the envs start an episode in every call
(another tenth each call).  Two ways, HIP events around each CALL (the windows are microseconds at 64 envs: call times, launches included,
not kernel times), two warm-up rounds, the two ways alternating in one process, medians over nine rounds of `--calls` calls each with the
smallest and the largest round next to them (the spread a difference has to beat):
  (a) the formula as torch tensor ops on the device, written here and fed the same tables: un-normalise, gather the ring rows, the update,
      torch.where for the fresh envs and the c == 0 rows, scatter back, the head row out, the counters -- ensemble; the queue: masks, gathers
      and torch.where;
  (b) chunks.ActionChunks.step.
The tool asserts that (a) and (b) agree to 1e-6 relative (torch's own rounding of the chain is not specified; tests/test_gpu_chunks.py
compares (b) with the specification for equality).  Bytes the ensemble pass must move: the chunk read, the ring read and written,
3 N C A 4, plus the action N A 4; (b)'s rate is those bytes over the time of the call, against the 8 TB/s HBM roof.  The queue moves
k A floats per env that takes a chunk and A per env otherwise; its rate is not stated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ROOF = 8e12
PEG = "gym_guided_vision/InsertPeg-3Arms-v0"


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "rounds": len(ms)}


class TorchEnsemble:
    """mode "ensemble" of av_aloha_amd/chunks.py as tensor ops"""

    def __init__(self, torch, N, C, A, tables, mean, std, dev):
        self.torch, self.N, self.C = torch, N, C
        self.w, self.cum = (torch.from_numpy(t.copy()).to(dev) for t in tables)
        self.mean, self.std = mean, std
        self.ens = torch.zeros((N, C, A), dtype=torch.float32, device=dev)
        self.head = torch.zeros(N, dtype=torch.int64, device=dev)
        self.count = torch.zeros(N, dtype=torch.int64, device=dev)
        self.last_id = torch.full((N,), -1, dtype=torch.int64, device=dev)
        self.k = torch.arange(C, dtype=torch.int64, device=dev)[None, :]
        self.env = torch.arange(N, dtype=torch.int64, device=dev)

    def step(self, x, ids, elapsed):
        torch, C = self.torch, self.C
        y = x * self.std + self.mean
        fresh = (elapsed == 0) | (ids != self.last_id)
        head, count = torch.where(fresh, 0, self.head), torch.where(fresh, 0, self.count)
        c = torch.minimum(count[:, None], C - 1 - self.k)
        j = ((head[:, None] + self.k) % C)[:, :, None].expand(-1, -1, y.shape[2])
        old = torch.gather(self.ens, 1, j)
        upd = (old * self.cum[(c - 1).clamp(min=0)][:, :, None] + y * self.w[c][:, :, None]) / self.cum[c][:, :, None]
        self.ens.scatter_(1, j, torch.where((c == 0)[:, :, None], y, upd))
        action = self.ens[self.env, head]
        self.head, self.count, self.last_id = (head + 1) % C, (count + 1).clamp(max=C - 1), ids.clone()
        return action


class TorchQueue:
    """mode "queue" as tensor ops, a chunk given in every call"""

    def __init__(self, torch, N, C, A, k, first, mean, std, dev):
        self.torch, self.kq, self.first = torch, k, first
        self.mean, self.std = mean, std
        self.q = torch.zeros((N, k, A), dtype=torch.float32, device=dev)
        self.row = torch.zeros(N, dtype=torch.int64, device=dev)
        self.left = torch.zeros(N, dtype=torch.int64, device=dev)
        self.last_id = torch.full((N,), -1, dtype=torch.int64, device=dev)
        self.env = torch.arange(N, dtype=torch.int64, device=dev)

    def step(self, x, ids, elapsed):
        torch = self.torch
        fresh = (elapsed == 0) | (ids != self.last_id)
        need = fresh | (self.left == 0)
        y = x[:, self.first:self.first + self.kq] * self.std + self.mean
        self.q = torch.where(need[:, None, None], y, self.q)
        row = torch.where(need, 0, self.row)
        action = self.q[self.env, row]
        self.row, self.left, self.last_id = row + 1, torch.where(need, self.kq, self.left) - 1, ids.clone()
        return action


def bench(N, C, A, k, calls, rounds, warmup):
    import numpy as np
    import torch
    from av_aloha_amd import chunks as ck
    from av_aloha_amd.vec_env import make_vec
    env = make_vec(PEG, N, 1000, cameras=[])
    dev = env.device
    rng = np.random.default_rng(N)
    stats = {"action": {"mean": rng.standard_normal(A).astype(np.float32), "std": (rng.random(A) + 0.25).astype(np.float32)}}
    mean, std = (torch.from_numpy(stats["action"][n]).to(dev) for n in ("mean", "std"))
    x = torch.from_numpy(rng.standard_normal((4, N, C, A)).astype(np.float32)).to(dev)
    # call t: env e starts an episode when (e + t) % 10 == 0
    e = np.arange(N)
    ids = [torch.from_numpy(e + N * ((e + t) // 10)).to(dev) for t in range(calls)]
    elapsed = [torch.from_numpy(((e + t) % 10).astype(np.int32)).to(dev) for t in range(calls)]
    infos = [{"episode_id": ids[t], "elapsed_steps": elapsed[t]} for t in range(calls)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {}
    for mode in ("ensemble", "queue"):
        kw = dict(ensemble=0.01) if mode == "ensemble" else dict(n_action_steps=k)
        ac = ck.ActionChunks(env, C, A, stats=stats, **kw)
        if mode == "ensemble":
            ta = TorchEnsemble(torch, N, C, A, ck.ensemble_tables(C, 0.01), mean, std, dev)
        else:
            ta = TorchQueue(torch, N, C, A, k, 0, mean, std, dev)
        # agreement over one pass of the calls
        worst = 0.0
        for t in range(calls):
            a, b = ta.step(x[t % 4], ids[t], elapsed[t]), ac.step(x[t % 4], infos[t])
            worst = max(worst, float(((a - b).abs() / b.abs().clamp(min=1e-3)).max()))
        assert worst <= 1e-6, f"{mode}: torch ops and avsim_chunk_step differ by {worst} relative"
        t_ms = {"a_torch": [], "b_chunk_step": []}
        for r in range(warmup + rounds):
            for key, way in (("a_torch", lambda t: ta.step(x[t % 4], ids[t], elapsed[t])), ("b_chunk_step", lambda t: ac.step(x[t % 4], infos[t]))):
                per_call = []
                for t in range(calls):
                    ev[0].record()
                    way(t)
                    ev[1].record()
                    torch.cuda.synchronize()
                    per_call.append(ev[0].elapsed_time(ev[1]))
                if r >= warmup:
                    t_ms[key].append(statistics.median(per_call))
        med = statistics.median(t_ms["b_chunk_step"])
        out = {**{key: summary(v) for key, v in t_ms.items()}, "a_over_b": statistics.median(t_ms["a_torch"]) / med,
               "a_spread": (max(t_ms["a_torch"]) - min(t_ms["a_torch"])) / statistics.median(t_ms["a_torch"]),
               "b_spread": (max(t_ms["b_chunk_step"]) - min(t_ms["b_chunk_step"])) / med, "max_rel_diff": worst, "calls_per_round": calls}
        if mode == "ensemble":
            moved = 3 * N * C * A * 4 + N * A * 4
            out.update({"b_bytes_moved": moved, "b_rate_TBps": moved / (med * 1e-3) / 1e12, "b_rate_over_hbm_roof": moved / (med * 1e-3) / HBM_ROOF})
        res[mode] = out
        print(N, mode, json.dumps(out), flush=True)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,1024,4096")
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--dim", type=int, default=21)
    ap.add_argument("--queue-steps", type=int, default=None, help="n_action_steps of the queue case (default: half the chunk)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tag", default="dev")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_chunks: no GPU -- the measurement has no CPU form")
    torch.zeros(1, device="cuda")
    k = args.queue_steps or max(1, args.chunk // 2)
    res = {"device": torch.cuda.get_device_name(0), "chunk": args.chunk, "dim": args.dim, "queue_steps": k, "envs": {}}
    for n in (int(v) for v in args.envs.split(",")):
        res["envs"][str(n)] = bench(n, args.chunk, args.dim, k, args.calls, args.rounds, args.warmup)
    path = args.out or os.path.join(ROOT, "profiles", f"chunks_{args.tag}.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
