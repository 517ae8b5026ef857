"""What the test_gpu_* modules share: torch with its HIP runtime up first, device-mode handles, the insert_peg fixtures and the
sentinel-guarded output.  A plain module: a test module imports it at its top, before it creates any handle, and imports the fixtures it
uses by name.  (The numpy-only helpers are in avsim_test_util.py.)"""
import numpy as np
import pytest
import torch

from av_aloha_amd import _ffi
from av_aloha_amd.sim import BatchedSim
from avsim_test_util import blob

# torch ships its own HIP runtime next to the one libavsim links: the vector env (vec_env.py) needs torch's to come up before libavsim's
# in a process, so this module brings it up when pytest imports the test module, before any test of the session has created a handle.
if torch.cuda.is_available():
    torch.zeros(1, device="cuda")


def device_handle(task="insert_peg", num_envs=2, flags=0, num_arms=3):
    """(a device-mode Handle on torch's current device, bound to torch's current stream; that torch.device).  The caller closes it."""
    d = torch.device("cuda", torch.cuda.current_device())
    h = _ffi.Handle(blob(task, num_arms), num_envs, d.index, flags | _ffi.AVSIM_IO_DEVICE)
    h.check(h.L.avsim_set_stream(h.h, torch.cuda.current_stream().cuda_stream))
    return h, d


def device_handle_in_state(task, num_envs, obj_poses, qpos, flags=0, num_arms=3):
    """device_handle, reset with those object poses [N, nobj * 7], then set to that qpos [N, nq], and synchronised."""
    h, d = device_handle(task, num_envs, flags, num_arms)
    obj = torch.from_numpy(np.ascontiguousarray(obj_poses)).to(d)
    h.check(h.L.avsim_reset(h.h, None, obj.data_ptr()))
    q = torch.from_numpy(np.ascontiguousarray(qpos)).to(d)
    h.check(h.L.avsim_set_qpos(h.h, q.data_ptr()))
    torch.cuda.synchronize()
    return h, d


@pytest.fixture(scope="module")
def sim():
    """A host-pointer BatchedSim: insert_peg, 3 arms, 2 envs.  Module-scoped: every module that imports it gets its own."""
    s = BatchedSim("insert_peg", 3, 2)
    yield s
    s.close()


@pytest.fixture(scope="module")
def dev():
    """(Handle, torch.device) of device_handle(): insert_peg, 3 arms, 2 envs.  Module-scoped: every module that imports it gets its own."""
    h, d = device_handle()
    yield h, d
    h.close()


class Guarded:
    """An output of `count` elements in the middle of a tensor filled with `sentinel` (a value of `dtype`): `lead` elements before it and
    `tail` after it, which a call that keeps to its output leaves alone.  Works on any device, the CPU included."""

    def __init__(self, device, count, dtype, sentinel, lead, tail):
        self.count, self.lead, self.sentinel = count, lead, sentinel
        self.whole = torch.full((lead + count + tail,), sentinel, dtype=dtype, device=device)

    def ptr(self, offset=0):
        """The address of the output, plus `offset` bytes."""
        return self.whole.data_ptr() + self.lead * self.whole.element_size() + offset

    def read(self):
        """(the output as numpy, every element outside it is still the sentinel, every element of it is still the sentinel).  The
        caller has synchronised."""
        w = self.whole.cpu().numpy()
        body = w[self.lead:self.lead + self.count]
        around = np.concatenate([w[:self.lead], w[self.lead + self.count:]])
        return body, bool((around == self.sentinel).all()), bool((body == self.sentinel).all())
