import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def blob(task="slot_insertion", num_arms=3):
    return open(os.path.join(ROOT, "models", f"{task}_{num_arms}arms.avm"), "rb").read()


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def noise(shape, seed):
    """u8 noise of that shape."""
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def same(a, b):
    """Both float32, of one shape, no NaN in either, and np.array_equal: equality of bits, -0 and +0 aside."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


def bits(a):
    """The uint32 bit patterns of a as float32: -0 and +0 differ, a NaN equals itself."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rand_quat(rng, small):
    if small:
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        ang = rng.uniform(-0.3, 0.3)
        return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def host_observe(sim):
    """agent_pos [N, nj] float64 of a host-pointer BatchedSim."""
    ap = np.empty((sim.N, sim.nj))
    sim.h.check(sim.h.L.avsim_observe(sim.h.h, ap.ctypes.data, None, None))
    return ap
