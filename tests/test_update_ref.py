"""CPU: the update audit's host-side pieces.

* the pure-Python reference (tests/update_ref.py) is self-consistent: Horner equals the naive power
  sum, and the difference predicted from the touched rows is the difference of the two files' values;
* lcpc_pos_update_rows (host only) follows the Python row-range rule over the corner grid;
* without a HIP device the new compute entries fail with LCPC_ERR_NO_DEVICE (no CPU fallback).
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import update_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")
INVALID_ARG, NO_DEVICE = 30, 33


@pytest.fixture(scope="module")
def lib():
    from lcpc_proof_of_storage_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", PKG], check=True)
    return N.load()


def grid():
    """(old_len, offset, length, pre) over the corners the issue names."""
    for pre in (4, 8):
        row = 7 * pre
        for old_len in (1, row - 1, row, 3 * row + 5):
            offsets = sorted({o for o in (0, 1, 6, 7, row - 1, row, old_len - 1, old_len) if 0 <= o <= old_len})
            for offset, length in itertools.product(offsets, (1, 6, 7, 8, row, row + 1, 3 * row)):
                yield old_len, offset, length, pre


def test_horner_equals_naive_power_sum():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 9, 100):
        coeffs = [int(v) for v in rng.integers(0, 1 << 56, n)]
        for x in (0, 1, R.P - 1, 1234567890123456789 % R.P):
            for d in (0, 1, (1 << 32) + 5, (1 << 64) - 1):
                assert R.horner(coeffs, x, d) == R.naive(coeffs, x, d)
    assert R.horner([5, 7], 0, 0) == 5 and R.horner([5, 7], 0, 3) == 0


def test_pack7_is_little_endian_and_zero_padded():
    assert R.pack7(b"") == []
    assert R.pack7(bytes(range(1, 9))) == [int.from_bytes(bytes(range(1, 8)), "little"), 8]


def test_expected_difference_is_the_difference_of_the_files():
    rng = np.random.default_rng(2)
    x = 0x1234567890ABCDEF % R.P
    for old_len, offset, length, pre in grid():
        old = rng.integers(0, 256, old_len, dtype=np.uint8).tobytes()
        data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        new = R.apply_update(old, offset, data)
        want = (R.file_value(new, x) - R.file_value(old, x)) % R.P
        assert R.expected_difference(old, offset, data, pre, x) == want, (old_len, offset, length, pre)


def _update_rows(lib, old_len, offset, length, pre):
    r = [C.c_size_t() for _ in range(4)]
    st = lib.lcpc_pos_update_rows(old_len, offset, length, pre, *[C.byref(v) for v in r])
    return st, tuple(v.value for v in r)


def test_update_rows_matches_the_python_rule(lib):
    n = 0
    for old_len, offset, length, pre in grid():
        st, got = _update_rows(lib, old_len, offset, length, pre)
        assert st == 0 and got == R.update_rows(old_len, offset, length, pre), (old_len, offset, length, pre)
        row_lo, row_hi, old_lo, old_hi = got
        assert row_lo < row_hi and old_lo <= old_hi <= old_len
        if offset == old_len and old_len % (7 * pre) == 0:
            assert old_lo == old_hi  # an append that starts a fresh row has no old bytes
        n += 1
    assert n > 300


def test_update_rows_rejects(lib):
    assert _update_rows(lib, 100, 10, 0, 4)[0] == INVALID_ARG     # len == 0
    assert _update_rows(lib, 100, 101, 1, 4)[0] == INVALID_ARG    # offset > old_len
    assert R.update_rows(100, 10, 0, 4) is None and R.update_rows(100, 101, 1, 4) is None


def test_new_compute_entries_need_a_device(lib):
    from lcpc_proof_of_storage_amd import lcpc2d
    if lcpc2d.device_count() > 0:
        pytest.skip("a HIP device is visible; the GPU tests cover these entries")
    u64p = C.POINTER(C.c_uint64)
    c = np.arange(1, 9, dtype=np.uint64)
    x, out = np.ones(1, np.uint64), np.zeros(8, np.uint64)
    data = np.arange(56, dtype=np.uint8)
    pc, px, po = (a.ctypes.data_as(u64p) for a in (c, x, out))
    calls = [
        lambda: lib.lcpc_eval_poly(0, pc, 8, px, 0, po),
        lambda: lib.lcpc_eval_poly_device(0, c.ctypes.data, 8, px, 0, po),
        lambda: lib.lcpc_pos_eval_poly_bytes(data.ctypes.data, 56, px, 0, po),
        lambda: lib.lcpc_pos_eval_poly_bytes_device(c.ctypes.data, 56, px, 0, po),
        lambda: lib.lcpc_pos_left_multiply_bytes(data.ctypes.data, 56, 8, px, 1, po),
        lambda: lib.lcpc_pos_left_multiply_bytes_device(c.ctypes.data, 56, 8, px, 1, po),
    ]
    for fn in calls:
        assert fn() == NO_DEVICE
