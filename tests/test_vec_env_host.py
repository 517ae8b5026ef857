"""Host side of the device-resident vector env (av_aloha_amd/vec_env.py): the numpy restatement of the library's Philox sampler, the
object-box table against the reference's draws, and the new C-ABI symbols."""
import ctypes as C

import numpy as np
import pytest

from av_aloha_amd.env import sample_object_poses
from av_aloha_amd.vec_env import OBJECT_BOXES, philox4x32_10, sample_poses

TASKS = ("insert_peg", "slot_insertion", "sew_needle", "tube_transfer", "hook_package")
NEW_SYMBOLS = ("avsim_episode_setup", "avsim_sample_poses", "avsim_episode_reset", "avsim_episode_step", "avsim_episode_log",
               "avsim_episode_count", "avsim_render_rgb_f32")


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors)."""
    z = philox4x32_10(np.zeros(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64))
    assert [f"{int(v):08x}" for v in z] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = philox4x32_10(np.full(4, 0xFFFFFFFF, dtype=np.uint64), np.full(2, 0xFFFFFFFF, dtype=np.uint64))
    assert [f"{int(v):08x}" for v in f] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


@pytest.mark.parametrize("task", TASKS)
def test_object_boxes_match_the_reference_draws(task):
    """20 000 draws of env.sample_object_poses (the reference's order from the global numpy RNG) lie inside the table's boxes, and every
    box is tight: the draws reach within 1 % of its width of both ends.  TubeTransfer's ball and tube1 share one draw."""
    box, share = (np.asarray(x) for x in OBJECT_BOXES[task])
    np.random.seed(1234)
    d = np.stack([sample_object_poses(task) for _ in range(20000)])
    assert d.shape[1] == len(share)
    lo, hi = np.minimum(box[:, :3], box[:, 3:]), np.maximum(box[:, :3], box[:, 3:])
    pos = d[:, :, :3]
    assert (pos >= lo).all() and (pos <= hi).all()
    w = hi - lo
    assert (pos.min(0) - lo <= 0.01 * w).all() and (hi - pos.max(0) <= 0.01 * w).all()
    assert (d[:, :, 3:] == [1.0, 0.0, 0.0, 0.0]).all()
    for o, s in enumerate(share):
        if s >= 0:
            assert np.array_equal(d[:, o], d[:, s])
    if task == "tube_transfer":
        assert list(share) == [-1, 0, -1]


@pytest.mark.parametrize("task", TASKS)
def test_philox_poses_lie_in_the_boxes_and_depend_on_seed_and_id_only(task):
    box, share = (np.asarray(x) for x in OBJECT_BOXES[task])
    ids = np.arange(5000)
    p = sample_poses(task, 7, ids)
    lo, hi = np.minimum(box[:, :3], box[:, 3:]), np.maximum(box[:, :3], box[:, 3:])
    assert (p[:, :, :3] >= lo).all() and (p[:, :, :3] <= hi).all()
    assert np.array_equal(sample_poses(task, 7, ids[::-1]), p[::-1])           # one id, one draw, whatever else is asked
    assert not np.array_equal(sample_poses(task, 8, ids)[:, :, :2], p[:, :, :2])
    for o, s in enumerate(share):
        if s >= 0:
            assert np.array_equal(p[:, o], p[:, s])


def test_new_symbols_are_exported_and_declared():
    from av_aloha_amd.build import build_hip
    from test_abi_symbols import declared_symbols
    L = C.CDLL(build_hip())
    decl = declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in decl, f"include/avsim.h does not declare {s}"
        assert hasattr(L, s), f"libavsim.so lacks {s}"
