"""The specification of the per-env observation histories (av_aloha_amd.obshist.ObsHistoryReference) against a literal restatement of LeRobot's
populate_queues, one deque per env; imgprep.history_index against a double loop; check_setup's refusals.  Host only."""
from collections import deque

import numpy as np
import pytest

from av_aloha_amd import imgprep
from av_aloha_amd import obshist as oh
from avsim_test_util import same


def fresh_schedule(N, calls):
    """env e is made fresh on call (e mod 5) + 1, in the way (e // 5) mod 5 names: by id change only, by elapsed == 0 only, by both, twice
    on consecutive calls, never.  (Call 0 starts every env: none has been pushed.)"""
    ids = np.zeros((calls, N), dtype=np.int64)
    elapsed = np.zeros((calls, N), dtype=np.int32)
    cur_id, cur_el = np.arange(N, dtype=np.int64), np.ones(N, dtype=np.int32)
    e = np.arange(N)
    when, way = e % 5 + 1, (e // 5) % 5
    for t in range(calls):
        hit = when == t
        again = (when + 1 == t) & (way == 3)
        new_id = (hit & np.isin(way, (0, 2, 3))) | again
        zero = hit & np.isin(way, (1, 2))
        cur_id = np.where(new_id, cur_id + N, cur_id)
        cur_el = np.where(zero, 0, cur_el)
        ids[t], elapsed[t] = cur_id, cur_el
        cur_el = cur_el + 1
    return ids, elapsed


class PopulateQueues:
    """LeRobot's populate_queues per env: a deque(maxlen=K) per env and key; an env that is fresh has its deques emptied (policy.reset()), and
    an empty deque is filled with K copies of the first observation; the policy reads torch.stack(list(queue), dim=1)."""

    def __init__(self, N, K, keys):
        self.N, self.K = N, K
        self.q = [{k: deque(maxlen=K) for k in keys} for _ in range(N)]
        self.seen = np.zeros(N, dtype=bool)
        self.last = np.zeros(N, dtype=np.int64)

    def push(self, new, ids, elapsed):
        out = {}
        for e in range(self.N):
            fresh = (not self.seen[e]) or elapsed[e] == 0 or ids[e] != self.last[e]
            for k, v in new.items():
                q = self.q[e][k]
                if fresh:
                    q.clear()
                if len(q) != self.K:
                    while len(q) != self.K:
                        q.append(v[e])
                else:
                    q.append(v[e])
        self.seen[:] = True
        self.last = np.array(ids, dtype=np.int64)
        for k in new:
            out[k] = np.stack([np.stack(list(self.q[e][k]), axis=0) for e in range(self.N)], axis=0)
        return out


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_reference_equals_populate_queues(K, fmt):
    N, D, H, W, h, w = 25, 5, 4, 7, 3, 6
    calls = 2 * K + 3
    rng = np.random.default_rng(K * 2 + fmt)
    ids, elapsed = fresh_schedule(N, calls)
    assert len({tuple(np.flatnonzero((elapsed[1:, e] == 0) | (ids[1:, e] != ids[:-1, e]))) for e in range(N)}) > 5
    mean, std = rng.standard_normal(D).astype(np.float32), (rng.random(D) + 0.25).astype(np.float32)
    lut = np.stack([imgprep.normalise_lut([0.4, 0.5, 0.6], [0.2, 0.25, 0.3]), imgprep.identity_lut()]).astype(np.float32)
    box = np.array([[1, 0, 1], [0, 1, 0]], dtype=np.int32)
    ref = oh.ObsHistoryReference(N, K, D, 2, fmt=fmt, src_hw=(H, W), out_hw=(h, w), lut=lut, box=box, mean=mean, std=std)
    lr = PopulateQueues(N, K, ["s", "i0", "i1"])
    for t in range(calls):
        state = rng.standard_normal((N, D)).astype(np.float32)
        u8 = [rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8) for _ in range(2)]
        imgs = u8 if fmt == 0 else [np.ascontiguousarray((u.astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)) for u in u8]
        sh, ih = ref.push(state, imgs, ids[t], elapsed[t])
        new = {"s": (state - mean) / std}
        for c in range(2):
            new[f"i{c}"] = imgprep.prep_reference(imgs[c], lut[c], None, np.tile(box[c], (N, 1)), (h, w))
        want = lr.push(new, ids[t], elapsed[t])
        assert same(sh, want["s"]) and same(ih[0], want["i0"]) and same(ih[1], want["i1"]), t
        if K == 1:
            assert same(ih[0][:, 0], new["i0"])


def test_a_fresh_env_holds_k_copies_and_reads_no_history():
    N, K, D = 3, 4, 2
    ref = oh.ObsHistoryReference(N, K, D)
    assert np.isnan(ref.state_hist).all()
    x = np.arange(N * D, dtype=np.float32).reshape(N, D)
    sh, ih = ref.push(x, None, [0, 1, 2], [0, 0, 0])
    assert ih == [] and same(sh, np.repeat(x[:, None], K, axis=1))
    sh, _ = ref.push(x + 10, None, [0, 1, 5], [1, 1, 1])
    assert same(sh[0], np.stack([x[0], x[0], x[0], x[0] + 10])) and same(sh[2], np.repeat(x[2:3] + 10, K, axis=0))
    ref.reset()
    assert ref.fresh([0, 1, 5], [2, 2, 2]).all()


def test_history_index_against_a_double_loop():
    ep_len = np.array([1, 2, 7], dtype=np.int64)
    ep_start = np.array([0, 1, 3], dtype=np.int64)
    frames = np.arange(10)
    for K in (1, 2, 3, 8):
        index, pad = imgprep.history_index(ep_start, ep_len, frames, K)
        assert index.dtype == np.int64 and pad.dtype == bool and index.shape == pad.shape == (10, K)
        for s, T in zip(ep_start, ep_len):
            for t in range(T):
                for k in range(K):
                    d = t - (K - 1) + k
                    assert index[s + t, k] == s + max(d, 0) and pad[s + t, k] == (d < 0), (K, s, t, k)
        assert np.array_equal(index[:, K - 1], frames) and not pad[:, K - 1].any()
    # any order, any subset
    index, pad = imgprep.history_index(ep_start, ep_len, [9, 1, 0], 3)
    assert index.tolist() == [[7, 8, 9], [1, 1, 1], [0, 0, 0]] and pad.tolist() == [[False] * 3, [True, True, False], [True, True, False]]
    with pytest.raises(IndexError):
        imgprep.history_index(ep_start, ep_len, [10], 2)
    with pytest.raises(IndexError):
        imgprep.history_index(ep_start, ep_len, [-1], 2)
    with pytest.raises(ValueError):
        imgprep.history_index(ep_start, ep_len, [0], 0)


def test_check_setup_refusals():
    lut = np.stack([imgprep.identity_lut()] * 2).astype(np.float32)
    box = np.array([[1, 1, 0], [0, 0, 1]], dtype=np.int32)
    cam = dict(ncam=2, fmt=0, src_hw=(5, 9), out_hw=(4, 8), lut=lut, box=box)
    ms, l, b = oh.check_setup(2, 3, mean=[0, 1, 2], std=[1, 2, 3], **cam)
    assert ms.shape == (2, 3) and ms.dtype == np.float32 and l.shape == (2, 3, 256) and b.dtype == np.int32 and np.array_equal(b, box)
    assert oh.check_setup(1, 0, **cam)[0] is None and oh.check_setup(16, 256)[1] is None

    def bad_box(c, j, v):
        x = box.copy()
        x[c, j] = v
        return x
    refused = [dict(K=0, D=3), dict(K=17, D=3), dict(K=2, D=-1), dict(K=2, D=257), dict(K=2, D=0), dict(K=2, D=3, ncam=-1), dict(K=2, D=3, ncam=9),
               dict(K=2, D=3, mean=[0, 0, 0]), dict(K=2, D=3, mean=[0, 0], std=[1, 1]), dict(K=2, D=3, mean=[0, np.nan, 0], std=[1, 1, 1]),
               dict(K=2, D=3, mean=[0, 0, 0], std=[1, 0, 1]), dict(K=2, D=3, mean=[0, 0, 0], std=[1, np.inf, 1]),
               dict(K=2, D=3, **{**cam, "fmt": 2}), dict(K=2, D=3, **{**cam, "fmt": "rgb"}), dict(K=2, D=3, **{**cam, "src_hw": (0, 9)}),
               dict(K=2, D=3, **{**cam, "src_hw": (5, 65536)}), dict(K=2, D=3, **{**cam, "out_hw": (0, 8)}), dict(K=2, D=3, **{**cam, "out_hw": (4, 65536)}),
               dict(K=2, D=3, **{**cam, "out_hw": (6, 8)}), dict(K=2, D=3, **{**cam, "box": bad_box(0, 0, 2)}), dict(K=2, D=3, **{**cam, "box": bad_box(1, 1, 2)}),
               dict(K=2, D=3, **{**cam, "box": bad_box(0, 0, -1)}), dict(K=2, D=3, **{**cam, "box": bad_box(1, 2, 2)}), dict(K=2, D=3, **{**cam, "box": bad_box(1, 2, -1)}),
               dict(K=2, D=3, **{**cam, "lut": lut[:1]}), dict(K=2, D=3, **{**cam, "box": box[:1]}), dict(K=2, D=3, **{**cam, "lut": None})]
    for kw in refused:
        with pytest.raises(ValueError):
            oh.check_setup(**kw)
    with pytest.raises(ValueError):
        oh.ObsHistoryReference(0, 2, 3)
    ref = oh.ObsHistoryReference(2, 2, 3, **{("cams" if k == "ncam" else k): v for k, v in cam.items()})
    with pytest.raises(ValueError):
        ref.push(np.zeros((2, 4), np.float32), [np.zeros((2, 5, 9, 3), np.uint8)] * 2, [0, 1], [0, 0])
    with pytest.raises(ValueError):
        ref.push(np.zeros((2, 3), np.float32), [np.zeros((2, 5, 9, 3), np.uint8)], [0, 1], [0, 0])
    with pytest.raises(ValueError):
        ref.push(np.zeros((2, 3), np.float32), [np.zeros((2, 3, 5, 9), np.float32)] * 2, [0, 1], [0, 0])
