"""The lane map of the paired contact-row fill (csrc/avsim_phys_layout.h: row_trips, rows_pair_pays, axis_rows), compiled for the host.

Env::make_constraints_i deals items 3 c + s -- axis s of contact c -- to the wave's lanes and lets axis_rows say which of the rows
first + s and first + s + 3 the lane fills; it takes that path only where rows_pair_pays.  What can go wrong is a row filled twice or
never, a lane reaching outside the contact rows, and a choice that costs trips.  The three models only hold condim 3 and 6: dims 1 and
4 are covered here and nowhere else."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = 64

SHIM = r"""
#include "avsim_phys_layout.h"
extern "C" int rp_trips(int n, int lanes) { return avs::row_trips(n, lanes); }
extern "C" int rp_pays(int ncon, int nrows, int lanes) { return avs::rows_pair_pays(ncon, nrows, lanes) ? 1 : 0; }
extern "C" int rp_axis(int ce, int s, int* row0, int* live1) {
    int r = -12345;
    bool l = false;
    const bool any = avs::axis_rows(ce, s, r, l);
    *row0 = r;
    *live1 = l ? 1 : 0;
    return any ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("rows_paired")
    src, so = d / "shim.cpp", d / "shim.so"
    src.write_text(SHIM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "av_aloha_amd", "csrc"),
                           "-o", str(so), str(src)])
    return ctypes.CDLL(str(so))


def row_table(dims, nlead0, maxefc):
    """The row words make_constraints_i leaves in cefc: contacts in order, dim 0 = inactive, a block that does not fit under the row cap
    dropped (-1; the offsets go on counting its rows, as on the device).  -> cefc list, nefc (end of the last kept block)"""
    cefc, first, nefc = [], nlead0, nlead0
    for dim in dims:
        if dim > 0 and first + dim <= maxefc:
            cefc.append(first | (dim << 16))
            nefc = max(nefc, first + dim)
        else:
            cefc.append(-1)
        first += dim
    return cefc, nefc


def visits(lib, cefc, ncon):
    """Rows visited by the paired loop, trip by trip, lane by lane -> list of rows, number of trips"""
    rows, trips = [], 0
    row0, live1 = ctypes.c_int(), ctypes.c_int()
    for base in range(0, 3 * ncon, LANES):
        trips += 1
        for lane in range(LANES):
            item = base + lane
            c, s = divmod(item, 3)
            ce = cefc[c] if c < ncon else -1
            if lib.rp_axis(ce, s, ctypes.byref(row0), ctypes.byref(live1)):
                rows.append(row0.value)
                if live1.value:
                    rows.append(row0.value + 3)
    return rows, trips


def check(lib, dims, nlead0, maxefc):
    ncon = len(dims)
    cefc, nefc = row_table(dims, nlead0, maxefc)
    rows, trips = visits(lib, cefc, ncon)
    want = [(ce & 0xffff) + k for ce in cefc if ce >= 0 for k in range(ce >> 16)]
    assert sorted(rows) == sorted(want), (dims, nlead0, maxefc)            # every row of every kept contact exactly once
    assert len(set(rows)) == len(rows)
    assert all(nlead0 <= i < nefc for i in rows), (dims, nlead0, maxefc)   # nothing outside the contact rows
    assert trips == lib.rp_trips(3 * ncon, LANES)
    old = lib.rp_trips(nefc - nlead0, LANES)
    new = trips if lib.rp_pays(ncon, nefc - nlead0, LANES) else old
    assert new <= old, (dims, nlead0, maxefc)                              # never more trips than one row per lane
    return old, new


@pytest.mark.parametrize("dim", [1, 3, 4, 6])
def test_uniform_dims_every_row_once(lib, dim):
    for ncon in range(49):
        for nlead0, maxefc in ((8, 1000), (0, 1000), (8, 8 + dim * ncon - (dim * ncon) // 3), (30, 40)):
            check(lib, [dim] * ncon, nlead0, maxefc)


def test_mixed_dims_inactive_contacts_and_the_row_cap(lib):
    rng = np.random.default_rng(7)
    saved = 0
    for ncon in range(49):
        for _ in range(6):
            dims = [int(d) for d in rng.choice([0, 1, 3, 4, 6], size=ncon, p=[0.1, 0.1, 0.3, 0.1, 0.4])]
            total = sum(dims)
            for maxefc in (1000, 8 + total, 8 + max(0, total - 5), 8 + total // 2, 16):
                old, new = check(lib, dims, 8, maxefc)
                saved += old - new
    assert saved > 0


def test_an_idle_axis_leaves_its_outputs_alone(lib):
    row0, live1 = ctypes.c_int(), ctypes.c_int()
    for ce, s in ((-1, 0), (-1, 2), (5 | (1 << 16), 1), (5 | (1 << 16), 2), (5 | (0 << 16), 0)):
        assert lib.rp_axis(ce, s, ctypes.byref(row0), ctypes.byref(live1)) == 0
        assert row0.value == -12345 and live1.value == 0
    # dim 4: axis 0 carries sub-rows 0 and 3, axes 1 and 2 one row each
    assert [(lib.rp_axis(20 | (4 << 16), s, ctypes.byref(row0), ctypes.byref(live1)), row0.value, live1.value) for s in range(3)] == [(1, 20, 1), (1, 21, 0), (1, 22, 0)]


def test_the_rule_on_the_benchmark_shapes(lib):
    assert lib.rp_pays(12, 72, LANES) == 1        # SlotInsertion at rest: 36 lanes, one trip instead of two
    assert lib.rp_pays(24, 128, LANES) == 0       # SewNeedle at rest: two trips either way -> one row per lane
    assert lib.rp_pays(21, 126, LANES) == 1 and lib.rp_pays(22, 128, LANES) == 0 and lib.rp_pays(22, 132, LANES) == 1
    assert lib.rp_pays(0, 0, LANES) == 0 and lib.rp_pays(10, 60, LANES) == 0
