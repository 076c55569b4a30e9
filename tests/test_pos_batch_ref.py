"""CPU: the batched stored-file audit's host-side pieces.

* the digit identity of the matrix-core kernel (csrc/pos_eval_mfma.hpp), restated in Python
  integers (tests/pos_batch_ref.py): signed file digits b - 128 against the balanced digits of
  left 2^(8a) mod p, plus the C128 term, give sum_r left[r] M[r][c]; and for the extreme inputs the
  GPU tests use, every accumulator of a 512-row split stays below the bound the kernel documents;
* the two _many entries report argument errors without a device, and a valid call answers
  LCPC_ERR_NO_DEVICE (no CPU fallback);
* lcpc_pos_left_multiply_many_kernel is a pure function of its arguments and LCPC_NO_MFMA.
"""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pos_batch_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")
INVALID_ARG, NO_DEVICE = 30, 33
PACK, VALU, MFMA = 0, 1, 2
BATCH_MAX = 4096
FILL = {0xff: (1 << 56) - 1, 0x00: 0, 0x80: 0x80808080808080, 0x7f: 0x7f7f7f7f7f7f7f}


@pytest.fixture(scope="module")
def lib():
    from lcpc_proof_of_storage_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", PKG], check=True)
    return N.load()


def test_balanced_digits_recompose():
    rng = random.Random(1)
    for w in [0, 1, B.P - 1, B.R % B.P] + [rng.randrange(B.P) for _ in range(50)]:
        for a, h in enumerate(B.h_digits(w)):
            assert all(-128 <= d < 128 for d in h)
            assert sum(d << (8 * u) for u, d in enumerate(h)) == (w << (8 * a)) % B.P


def test_digit_identity_random_rows():
    """512 rows of random words against random elements: the kernel's route equals the field sum."""
    rng = random.Random(2)
    left = [rng.randrange(B.P) for _ in range(512)]
    elems = [rng.randrange(1 << 56) for _ in range(512)]
    want = sum(lw * e for lw, e in zip(left, elems)) * B.RINV % B.P
    assert B.column_value(left, elems) == want
    assert max(abs(y) for y in B.accumulators(left, elems)) < B.Y_BOUND


@pytest.mark.parametrize("fill", sorted(FILL))
def test_digit_identity_and_bound_at_the_extremes(fill):
    """The GPU tests' extreme images (every byte 0xff, 0x00, 0x80, 0x7f) against 512 rows of p - 1,
    1, 0, R mod p and random words: the identity holds and the exact |Y| is below the bound."""
    rng = random.Random(3)
    elems = [FILL[fill]] * 512
    for name, left in (("p-1", [B.P - 1] * 512), ("1", [1] * 512), ("0", [0] * 512), ("R", [B.R % B.P] * 512),
                       ("random", [rng.randrange(B.P) for _ in range(512)])):
        Y = B.accumulators(left, elems)
        assert max(abs(y) for y in Y) < B.Y_BOUND, (fill, name, Y)
        assert max(abs(y) for y in Y) <= B.Y_MAX
        assert B.column_value(left, elems) == sum(left) * FILL[fill] * B.RINV % B.P, (fill, name)


def test_same_sign_rows_reach_half_the_bound():
    """One accumulator driven by products of one sign over 512 rows stays below the bound and
    reaches at least half of it (the words are picked for large digits at that position).  Position
    7 holds the top byte of a value below p, a digit in [0, 0x46]: it is held to half of what such
    digits can reach."""
    for u in (0, 3, 7):
        for mirror in (False, True):
            left, elems = B.same_sign_rows(u, 512, 40 + u, mirror=mirror)
            Y = B.accumulators(left, elems)
            assert abs(Y[u]) < B.Y_BOUND and 2 * abs(Y[u]) >= (B.reach(7) if u == 7 else B.Y_BOUND), \
                (u, mirror, Y[u] / B.Y_BOUND)
            assert (Y[u] > 0) != mirror
            assert B.column_value(left, elems) == sum(lw * e for lw, e in zip(left, elems)) * B.RINV % B.P


def test_recombine_offset_covers_the_bound():
    """recombine_redc63 adds p 2^21 to a signed sum of 8 positions of at most 2^26 each."""
    worst = sum(B.Y_BOUND << (8 * u) for u in range(8))
    assert B.P << 21 > worst
    assert (worst + (B.P << 21)) >> 64 < 1 << 20   # the top word added after the reduction
    assert B.P + (1 << 20) < 2 * B.P


def _ptrs(*arrays):
    return [a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrays]


def test_many_entries_report_argument_errors_without_a_device(lib):
    data = np.arange(7 * 8 * 3 - 2, dtype=np.uint8)          # 3 rows of pre = 8, the last ragged
    lefts, out = np.ones(2 * 3, np.uint64), np.zeros(2 * 8, np.uint64)
    pl, po = _ptrs(lefts, out)
    for fn, img in ((lib.lcpc_pos_left_multiply_bytes_many, data.ctypes.data),
                    (lib.lcpc_pos_left_multiply_bytes_many_device, lefts.ctypes.data)):
        assert fn(None, data.size, 8, pl, 2, 3, po) == INVALID_ARG
        assert fn(img, data.size, 8, None, 2, 3, po) == INVALID_ARG
        assert fn(img, data.size, 8, pl, 2, 3, None) == INVALID_ARG
        assert fn(img, 0, 8, pl, 2, 3, po) == INVALID_ARG
        assert fn(img, data.size, 0, pl, 2, 3, po) == INVALID_ARG
        assert fn(img, data.size, 8, pl, 0, 3, po) == INVALID_ARG
        assert fn(img, data.size, 8, pl, BATCH_MAX + 1, 3, po) == INVALID_ARG
        for n_left in (2, 4):
            assert fn(img, data.size, 8, pl, 2, n_left, po) == INVALID_ARG
    # a device image that is not 8-byte aligned
    assert lib.lcpc_pos_left_multiply_bytes_many_device(lefts.ctypes.data + 4, data.size, 8, pl, 2, 3, po) == INVALID_ARG
    assert lib.lcpc_selftest_recombine63(None, po, 1) == INVALID_ARG
    assert lib.lcpc_selftest_recombine63(np.zeros(8, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), None, 1) == INVALID_ARG


def test_valid_calls_need_a_device(lib):
    from lcpc_proof_of_storage_amd import lcpc2d
    if lcpc2d.device_count() > 0:
        pytest.skip("a HIP device is visible; the GPU tests cover these entries")
    data = np.arange(7 * 8 * 3 - 2, dtype=np.uint8)
    lefts, out = np.ones(2 * 3, np.uint64), np.zeros(2 * 8, np.uint64)
    pl, po = _ptrs(lefts, out)
    assert lib.lcpc_pos_left_multiply_bytes_many(data.ctypes.data, data.size, 8, pl, 2, 3, po) == NO_DEVICE
    assert lib.lcpc_pos_left_multiply_bytes_many_device(lefts.ctypes.data, data.size, 8, pl, 2, 3, po) == NO_DEVICE
    assert lib.lcpc_selftest_recombine63(np.zeros(8, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), po, 1) == NO_DEVICE


def _kernel_table(lib):
    return [lib.lcpc_pos_left_multiply_many_kernel(pre, m)
            for pre in (1, 7, 8, 16, 24, 32, 64, 96, 128, 16384) for m in (1, 2, 3, 16, 17, 4096)]


def test_kernel_choice_is_a_pure_function(lib):
    from lcpc_proof_of_storage_amd import pos
    table = _kernel_table(lib)
    assert table == _kernel_table(lib)
    for m in (1, 16, 4096):
        assert [lib.lcpc_pos_left_multiply_many_kernel(pre, m) for pre in (1, 7, 24, 96)] == [PACK] * 4
        assert [lib.lcpc_pos_left_multiply_many_kernel(pre, m) for pre in (8, 16, 32)] == [VALU] * 3
    assert pos.left_multiply_many_kernel(24, 3) == PACK and pos.left_multiply_many_kernel(16, 3) == VALU
    # the environment is the only other input: a child under LCPC_NO_MFMA=1 never names the matrix cores
    code = ("import sys; sys.path.insert(0, %r); from lcpc_proof_of_storage_amd import _native as N; l = N.load(); "
            "print([l.lcpc_pos_left_multiply_many_kernel(p, m) for p in (8, 24, 64, 16384) for m in (1, 16, 64)])" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LCPC_NO_MFMA="1"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert eval(r.stdout.strip()) == [VALU] * 3 + [PACK] * 3 + [VALU] * 6
