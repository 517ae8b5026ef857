"""The host cost of a C entry point's array staging (csrc/avsim_io.h), microseconds per call at 64 envs; prints one JSON line.  Run it
in two checkouts alternately to compare them (profiles/io_call.json: tools/exp_abba.sh's pattern).

    python tools/bench_io_call.py

* host_step_us: BatchedSim.step, host I/O, 20 substeps -- the call as a numpy user makes it.
* with nsub = 0, the shortest kernel, so that the host side shows: device_episode_step_nsub0_us (avsim_episode_step, one input and seven outputs,
  5000 calls enqueued and one synchronise), host_step_nsub0_us and host_get_state_us (2000 synchronous calls each).
Every figure is the best of three windows; the windows are printed too."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

N = 64


def best_of_3(n, fn, done=lambda: None):
    win = []
    for _ in range(3):
        t = time.perf_counter()
        for _ in range(n):
            fn()
        done()
        win.append((time.perf_counter() - t) / n * 1e6)
    return win


def main():
    import torch
    from av_aloha_amd.sim import BatchedSim
    from av_aloha_amd.vec_env import make_vec, sample_poses
    env = make_vec("gym_guided_vision/SlotInsertion-3Arms-v0", N, 300, cameras=[])
    env.reset(seed=0)
    a = env._ap.float().clone()
    h, L = env.h, env.L

    def episode_step():
        h.check(L.avsim_episode_step(h.h, a.data_ptr(), 0, env._ap.data_ptr(), env._reward.data_ptr(), env._success.data_ptr(), env._term.data_ptr(),
                                     env._trunc.data_ptr(), env._id.data_ptr(), env._elapsed.data_ptr()))
    for _ in range(500):
        episode_step()
    torch.cuda.synchronize()
    win = {"device_episode_step_nsub0_us": best_of_3(5000, episode_step, torch.cuda.synchronize)}
    env.close()

    s = BatchedSim("slot_insertion", 3, N)
    s.reset(sample_poses("slot_insertion", 1, list(range(N))))
    ap, _, _ = s.step(np.zeros((N, s.nj), np.float32), nsub=0)
    act = ap.astype(np.float32)
    for _ in range(200):
        s.step(act, nsub=0)
        s.get_state()
        s.step(act)
    win["host_step_nsub0_us"] = best_of_3(2000, lambda: s.step(act, nsub=0))
    win["host_get_state_us"] = best_of_3(2000, s.get_state)
    win["host_step_us"] = best_of_3(300, lambda: s.step(act))
    s.close()
    print(json.dumps({**{k: min(v) for k, v in win.items()}, "num_envs": N, "windows": win}))


if __name__ == "__main__":
    main()
