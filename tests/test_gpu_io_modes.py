"""Host I/O mode against device I/O mode: two handles of one model on one device, one fed numpy arrays and one (AVSIM_IO_DEVICE) torch tensors,
driven through the same calls.  After every call the host handle's arrays hold the bytes of the device handle's tensors -- outputs that were asked
for and ones that were not, an in-out canvas and in-out histories, outputs the handle keeps itself, a result that grows and shrinks again."""
import ctypes
import os

import numpy as np
import pytest

from av_aloha_amd import _ffi
from av_aloha_amd import workloads as W
from av_aloha_amd.compiler.compile import read_blob
from av_aloha_amd.constants import MODEL_DIR, SIM_PHYSICS_ENV_STEP_RATIO
from av_aloha_amd.vec_env import OBJECT_BOXES, sample_poses
from avsim_test_util import blob
from gpu_util import device_handle, torch as T

pytestmark = pytest.mark.gpu

TASK, N = "insert_peg", 3
CAMS = ["zed_cam_left", "overhead_cam"]


class Side:
    """One handle and the arrays it is fed: numpy (host I/O) or torch tensors on the handle's device (device I/O)."""

    def __init__(self, device_mode):
        self.T, self.device_mode = T, device_mode
        if device_mode:
            self.h, self.dev = device_handle(TASK, N)
        else:
            self.dev = T.device("cuda", T.cuda.current_device())
            self.h = _ffi.Handle(blob(TASK), N, self.dev.index)
        self.L = self.h.L

    def arr(self, a):
        a = np.ascontiguousarray(a).copy()
        return self.T.from_numpy(a.reshape(-1).view(np.uint8)).to(self.dev) if self.device_mode else a          # (a tensor of the array's bytes)

    def fresh(self, shape, dtype):
        """An output array, 0xAB in every byte: what a call leaves alone compares too."""
        return self.arr(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xAB, np.uint8).view(dtype).reshape(shape))

    def bytes(self, a):
        return a.cpu().numpy().tobytes() if self.device_mode else a.tobytes()

    def call(self, name, *args):
        self.h.check(getattr(self.L, name)(self.h.h, *[_ffi.ptr(a) if not isinstance(a, (bytes, ctypes.Array)) else a for a in args]))

    def close(self):
        self.h.close()


def drive(s):
    """The sequence on one side: yields (what was called, the arrays to compare) after every call."""
    rng = np.random.default_rng(11)
    md = read_blob(os.path.join(MODEL_DIR, f"{TASK}_3arms.avm"))
    nq, nv, nu, nj, nobj = s.h.nq, s.h.nv, s.h.nu, s.h.nj, s.h.nobj
    acts = W.walk_actions(md["qpos_home"], md["act_ctrlrange"], list(range(N)), 4, nj, 7000)
    names = json_cameras()
    ids = np.array([names.index(c) for c in CAMS], dtype=np.int32)          # (camera indices are host arrays in either mode)

    def state(tag):
        st = [s.fresh((N, n), np.float64) for n in (nq, nv, nu, nv)]
        s.call("avsim_get_state", *st)
        return tag, st

    # 1. reset with a mask
    s.call("avsim_reset", s.arr(np.array([1, 0, 1], np.uint8)), s.arr(sample_poses(TASK, 1, [0, 1, 2]).astype(np.float64)))
    yield state("get_state after reset(mask)")
    # 2. step without reward / success, then with every output
    ap, rw, su = s.fresh((N, nj), np.float64), s.fresh(N, np.int32), s.fresh(N, np.uint8)
    s.call("avsim_step", s.arr(acts[0]), SIM_PHYSICS_ENV_STEP_RATIO, ap, None, None)
    yield "step(agent_pos)", [ap, rw, su]
    s.call("avsim_step", s.arr(acts[1]), SIM_PHYSICS_ENV_STEP_RATIO, ap, rw, su)
    yield "step(all)", [ap, rw, su]
    # 3. the state
    yield state("get_state")

    # 4. depth images, 2 cameras at 8 x 12
    def depth(H, Wd):
        out = s.fresh((N, 2, H, Wd), np.float32)
        s.call("avsim_render_depth", ids, 2, H, Wd, out)
        return f"render_depth {H}x{Wd}", [out]
    yield depth(8, 12)
    # 5. statistics of a batch through an index
    batch = rng.integers(0, 256, (5, 8, 12, 3), dtype=np.uint8)
    stats = s.fresh((4, 12), np.uint64)
    s.call("avsim_image_stats", s.arr(batch), 0, s.arr(np.array([4, 0, 2, 2], np.int32)), 4, 8, 12, stats)
    yield "image_stats", [stats]
    # 6. compose into a canvas that holds something (in-out), then label it (in-out again)
    canvas = s.arr(rng.integers(0, 256, (2, 16, 24, 3), dtype=np.uint8))
    places = np.array([[0, 0, 1, 2, 12, 8], [0, 4, 14, 3, 9, 12], [1, 3, 5, 4, 18, 11]], np.int32)
    s.call("avsim_compose", s.arr(batch), 0, 5, 8, 12, canvas, 0, 2, 16, 24, places, len(places), 0, 0)
    yield "compose(clear=0)", [canvas]
    where = np.array([[0, 1, 1, 1], [1, 0, 8, 1]], np.int32)
    s.call("avsim_compose_label", canvas, 0, 2, 16, 24, where, 2, b"e", s.arr(np.array([7, 42], np.int64)), 0x20FF40)
    yield "compose_label", [canvas]
    # 7. observation histories: K = 2, the joints and one 8 x 12 camera cropped to 6 x 10, pushed twice (in-out histories)
    lut = rng.random((1, 3, 256), dtype=np.float32)
    s.call("avsim_obs_history_setup", 2, nj, None, 1, 0, 8, 12, lut, np.array([[1, 2, 1]], np.int32), 6, 10)
    shist = s.arr(np.full((N, 2, nj), np.nan, np.float32))
    ihist = s.arr(np.full((N, 2, 3, 6, 10), np.nan, np.float32))
    eid = s.arr(np.zeros(N, np.int64))
    for k in range(2):
        st = s.arr(rng.standard_normal((N, nj)).astype(np.float32))
        img = s.arr(batch[k:k + N])
        src, dst = (ctypes.c_void_p * 1)(_ffi.ptr(img)), (ctypes.c_void_p * 1)(_ffi.ptr(ihist))
        s.call("avsim_obs_history_push", eid, s.arr(np.full(N, k, np.int32)), st, shist, src, dst)
        yield f"obs_history_push {k}", [shist, ihist]
    # 8. an episode step whose terminated / truncated nobody asks for (the handle's own buffers)
    box, share = (np.ascontiguousarray(OBJECT_BOXES[TASK][0], dtype=np.float64), np.ascontiguousarray(OBJECT_BOXES[TASK][1], dtype=np.int32))
    assert box.shape == (nobj, 6)
    s.h.check(s.L.avsim_episode_setup(s.h.h, box.ctypes.data, share.ctypes.data, 1234, 50, 1, 0))
    ep_id, el = s.fresh(N, np.int64), s.fresh(N, np.int32)
    s.call("avsim_episode_step", s.arr(acts[2]), SIM_PHYSICS_ENV_STEP_RATIO, ap, rw, su, None, None, ep_id, el)
    yield "episode_step", [ap, rw, su, ep_id, el]
    s.call("avsim_episode_step", s.arr(acts[3]), SIM_PHYSICS_ENV_STEP_RATIO, ap, rw, su, None, None, ep_id, el)          # (the first one started the episodes)
    yield "episode_step 2", [ap, rw, su, ep_id, el]
    yield state("get_state after episode_step")
    # 9. a larger depth image, then the first size again (the staging grows, then serves the smaller result)
    yield depth(24, 16)
    yield depth(8, 12)


def json_cameras():
    import json
    with open(os.path.join(MODEL_DIR, f"{TASK}_3arms.json")) as f:
        return json.load(f)["camera_names"]


def test_host_and_device_handles_agree_byte_for_byte():
    host, dev = Side(False), Side(True)
    try:
        seen = []
        for (what, a), (what_d, b) in zip(drive(host), drive(dev)):
            assert what == what_d and len(a) == len(b)
            for i, (x, y) in enumerate(zip(a, b)):
                hx, dy = host.bytes(x), dev.bytes(y)
                assert len(hx) == len(dy) and hx == dy, f"{what}: array {i} differs between host and device I/O"
            # ... and the calls did something
            if what == "step(agent_pos)":
                assert np.isfinite(a[0]).all() and a[1].tobytes() == b"\xab" * (4 * N) and a[2].tobytes() == b"\xab" * N
            if what == "step(all)":
                assert (a[1] >= 0).all() and (a[2] <= 1).all()
            if what.startswith("render_depth"):
                assert np.isfinite(a[0]).all() and a[0].std() > 0
            if what.startswith("obs_history_push"):
                assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
            if what == "episode_step":
                assert a[3].tolist() == [0, 1, 2] and a[4].tolist() == [0, 0, 0]
            if what == "episode_step 2":
                assert a[3].tolist() == [0, 1, 2] and a[4].tolist() == [1, 1, 1]
            seen.append(what)
        assert len(seen) == 15 and len(set(seen)) == 14, seen          # (render_depth 8x12 comes twice)
    finally:
        host.close()
        dev.close()
