"""What tests/test_segment_host.py and tests/test_gpu_segment.py share (test infrastructure only): the states and cameras the label image
is compared in, the reference cast of the nine rays of every pixel, and the comparison rule.

The rule.  With K = K_PROXY = 5 the reference (av_aloha_amd.segment.cast_reference, f64) is cast at K H x K W; the centre of pixel (i, j)
is the centre of high-resolution pixel (K i + 2, K j + 2) and its eight neighbours there are the rays 1 / K pixel off the centre
(tests/render_envelope.py).  The ACCEPTED labels of a pixel are table[g] of every geom whose entry depth is within TOL_DEPTH of the nearest
one at any of those nine rays, and the background where any of the nine meets nothing.  A device pixel with one accepted label must carry
it; one with several must carry one of them, apart from at most one per image and one per 10 000 compared pixels (Tally's edge allowance:
a surface narrower than 1 / K pixel can pass between the nine rays, nothing else can)."""
import numpy as np

import render_envelope as RE
from av_aloha_amd import segment

K = RE.K_PROXY
SIZES = [(30, 40), (33, 42), (24, 332)]       # one partly filled tile, 32-bit label stores | W % 4 != 0, three tile rows over two bin rows | 11 tiles across, two bin columns
MIN_SINGLE = 0.75                             # of an image's pixels have exactly one accepted label: the rule's precondition
# (task, the three states of the batch, [(env, camera)] compared)
GROUPS = [("slot_insertion", ("S0", "S3", "S5"), [(0, "zed_cam_left"), (1, "wrist_cam_left"), (2, "overhead_cam")]),
          ("slot_insertion", ("S1", "S3", "S5"), [(0, "zed_cam_left")]),
          ("hook_package", ("R0", "R2", "R1"), [(1, "wrist_cam_right")]),
          ("tube_transfer", ("R0", "R2", "R1"), [(1, "wrist_cam_right")])]
CASES = [(task, states, env, cam) for task, states, views in GROUPS for env, cam in views]
HOST_SLOT = ["S0", "S1", "S2", "S3", "S5"]
HOST_CAMS = ["zed_cam_left", "wrist_cam_left", "wrist_cam_right", "overhead_cam"]


def states_of(task, e):
    """{name: qpos}: render_envelope's states of the task; R1 (the other tasks) is the reset pose with the left arm's shoulder turned, a
    third state for a batch of three."""
    if task == "slot_insertion":
        return RE.slot_states(e)
    S = RE.other_task_states(task, e)
    S["R1"] = S["R0"].copy()
    S["R1"][1] += 0.2
    return S


def oracle_cast(md, e, cam, H, W, rows=None, cols=None):
    """cast_reference of the oracle's current state."""
    ng, nb = len(e.man["geom_names"]), md["nbody"]
    ci = e.man["camera_names"].index(cam)
    pc, Rc = segment.camera_pose(md, e.arr("xpos", 3 * nb), e.arr("xmat", 9 * nb), ci)
    return segment.cast_reference(md, e.arr("geom_xpos", 3 * ng).copy(), e.arr("geom_xmat", 9 * ng).copy(), pc, Rc, ci, H, W, rows=rows, cols=cols)


def nine_rays(md, e, cam, H, W):
    """float64 [ngeom, H, 3, W, 3]: the entry depths along the nine rays of every pixel (only those of the K H x K W grid are cast)."""
    c = K // 2
    rows = (K * np.arange(H)[:, None] + c + np.arange(-1, 2)[None, :]).reshape(-1)
    cols = (K * np.arange(W)[:, None] + c + np.arange(-1, 2)[None, :]).reshape(-1)
    cast = oracle_cast(md, e, cam, K * H, K * W, rows, cols)
    return cast.reshape(len(cast), H, 3, W, 3)


def accepted(rays, table, zfar=RE.FAR, tol=RE.TOL_DEPTH):
    """bool [256, H, W]: accepted[l, i, j] -- label l is accepted at pixel (i, j)."""
    ng, H, _, W, _ = rays.shape
    near = rays.min(axis=0)
    acc = np.zeros((256, H, W), dtype=bool)
    acc[int(table[ng])] = (near >= zfar).any(axis=(1, 3))
    for g in range(ng):
        close = (rays[g] <= near + tol) & (rays[g] < zfar)
        if close.any():
            acc[int(table[g])] |= close.any(axis=(1, 3))
    return acc


class LabelTally:
    """The rule over one test function: add() every image, then done()."""

    def __init__(self):
        self.compared = self.single_bad = self.multi_bad = 0
        self.failed, self.lines = False, []

    def add(self, img, acc, label):
        assert img.shape == acc.shape[1:], (label, img.shape, acc.shape)
        H, W = img.shape
        ok = acc[img.astype(np.int64), np.arange(H)[:, None], np.arange(W)[None, :]]
        single = acc.sum(axis=0) == 1
        ns, nm = int((~ok & single).sum()), int((~ok & ~single).sum())
        self.compared += img.size
        self.single_bad += ns
        self.multi_bad += nm
        if ns or nm > 1:
            self.failed = True
        for i, j in np.argwhere(~ok)[:12]:
            self.lines.append(f"{label} pixel ({i}, {j}) tile ({i // RE.TILE_H}, {j // RE.TILE_W}): device {img[i, j]} accepted {np.flatnonzero(acc[:, i, j]).tolist()}")
        return ns, nm

    def done(self):
        if self.lines:
            print("\n".join(self.lines))
        assert not self.failed and self.multi_bad * 10000 <= self.compared, (
            f"{self.single_bad} pixels with one accepted label and {self.multi_bad} with several carry another, in {self.compared} compared "
            f"(allowed: none; one per image and one per 10 000 in all)\n" + "\n".join(self.lines))


def single_share(acc):
    return float((acc.sum(axis=0) == 1).mean())
