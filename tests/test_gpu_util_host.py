"""The checks the GPU tests share (tests/gpu_util.py Guarded, tests/avsim_test_util.py same / bits) still bite: on CPU tensors, with
ctypes writing through the pointer the helper hands out, as a kernel would through the device pointer."""
import ctypes

import numpy as np
import pytest

from avsim_test_util import bits, same
from gpu_util import Guarded, torch

COUNT, TAIL = 37, 1024
# (dtype, sentinel, lead): words on and off a 16-byte boundary, as the image tests alternate them; bytes that start at an odd offset
KINDS = [(torch.int32, 0xA5A5A5A5 - (1 << 32), 1024), (torch.int32, 0xA5A5A5A5 - (1 << 32), 1021), (torch.uint8, 0x5A, 1021)]
IDS = ["words-1024", "words-1021", "bytes-1021"]


def guarded(kind):
    dtype, sentinel, lead = kind
    g = Guarded("cpu", COUNT, dtype, sentinel, lead, TAIL)
    return g, g.whole.element_size()


@pytest.mark.parametrize("where", ["before", "after", "far end"])
@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_guarded_reports_one_element_written_outside_the_output(kind, where):
    g, size = guarded(kind)
    element = {"before": -1, "after": COUNT, "far end": COUNT + TAIL - 1}[where]
    ctypes.memset(g.ptr(element * size), 0, size)
    body, intact, untouched = g.read()
    assert not intact
    assert untouched and len(body) == COUNT


@pytest.mark.parametrize("kind", KINDS, ids=IDS)
def test_guarded_raises_no_false_alarm(kind):
    g, size = guarded(kind)
    body, intact, untouched = g.read()
    assert intact and untouched and (body == kind[1]).all()
    src = np.arange(1, COUNT + 1).astype(body.dtype)
    ctypes.memmove(g.ptr(), src.ctypes.data, COUNT * size)
    body, intact, untouched = g.read()
    assert intact and not untouched and np.array_equal(body, src)
    # the first and the last element alone: still inside
    g, size = guarded(kind)
    ctypes.memset(g.ptr(), 0, size)
    ctypes.memset(g.ptr((COUNT - 1) * size), 0, size)
    body, intact, untouched = g.read()
    assert intact and not untouched and body[0] == 0 and body[-1] == 0 and (body[1:-1] == kind[1]).all()
    assert g.ptr(3) == g.ptr() + 3 and g.ptr() == g.whole.data_ptr() + kind[2] * size


def test_same_and_bits():
    a = np.array([[1.5, -2.0, 0.0], [3.0, 4.0, 1e-30]], dtype=np.float32)
    assert same(a, a.copy())
    nan = a.copy()
    nan[1, 2] = np.nan
    assert not same(nan, a) and not same(a, nan) and not same(nan, nan.copy())
    assert not same(a.astype(np.float64), a) and not same(a, a.astype(np.float64)) and not same(a.astype(np.float64), a.astype(np.float64))
    assert not same(a.reshape(3, 2), a) and not same(a[:, :2], a)
    other = a.copy()
    other[0, 0] = np.nextafter(np.float32(1.5), np.float32(2))
    assert not same(other, a)
    minus = a.copy()
    minus[0, 2] = -0.0
    assert same(minus, a)                                  # -0 and +0 are equal to `same` ...
    assert not np.array_equal(bits(minus), bits(a))        # ... and differ in their bits
    assert np.array_equal(bits(a), bits(a.copy())) and bits(a).dtype == np.uint32 and np.array_equal(bits(nan), bits(nan.copy()))
