"""GPU: the streaming polynomial evaluation and the byte-image left multiply (pos_eval.hip) against
Python integers and the oracle.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import update_ref as R
from pyref import FIELD_DECL

pytestmark = pytest.mark.gpu
FT63 = 0
INVALID_ARG = 30


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    return N.load()


def _points(oracle, fid):
    p = FIELD_DECL[fid][0]
    rnd = oracle.ChaCha(seed_u64=77 + fid).field_random(fid, 1)
    return [oracle.to_mont(fid, [0]), oracle.to_mont(fid, [1]), oracle.to_mont(fid, [p - 1]), rnd]


DEGREES = (0, 1, (1 << 32) + 5, (1 << 64) - 1)


@pytest.mark.parametrize("fid", [0, 1, 2, 3, 4])
def test_eval_poly_elements(pos, oracle, hipmem, native, fid):
    """Every n around a lane stride (256) and the block tile T, x in {0, 1, p - 1, random}, every
    kind of degree offset; the device entry gives the host entry's words."""
    T, p, nl = pos.EVAL_POLY_TILE, FIELD_DECL[fid][0], oracle.limbs(fid)
    coeffs = oracle.random_coeffs(fid, T + 1, 500 + fid)
    canon = oracle.from_mont(fid, coeffs)
    for x in _points(oracle, fid):
        xv = oracle.from_mont(fid, x)[0]
        for n in (0, 1, 2, 255, 256, 257, T - 1, T, T + 1):
            for d in DEGREES:
                got = pos.evaluate_field_polynomial_at_point_with_elevated_degree(coeffs[:n * nl], x, d, fid)
                assert oracle.from_mont(fid, got.reshape(-1))[0] == R.horner(canon[:n], xv, d, p), (n, xv, d)
    x = _points(oracle, fid)[3]
    want = pos.evaluate_field_polynomial_at_point_with_elevated_degree(coeffs, x, 3, fid)
    dev = hipmem.to_device(coeffs)
    out = np.zeros(nl, np.uint64)
    try:
        st = native.lcpc_eval_poly_device(fid, dev, T + 1, x.ctypes.data_as(C.POINTER(C.c_uint64)), 3,
                                          out.ctypes.data_as(C.POINTER(C.c_uint64)))
    finally:
        hipmem.free(dev)
    assert st == 0 and np.array_equal(out, want.reshape(-1))


def test_eval_poly_plain_is_degree_zero(pos, oracle):
    c = oracle.random_coeffs(FT63, 300, 9)
    x = oracle.ChaCha(seed_u64=3).field_random(FT63, 1)
    assert np.array_equal(pos.evaluate_field_polynomial_at_point(c, x),
                          pos.evaluate_field_polynomial_at_point_with_elevated_degree(c, x, 0))
    zero = oracle.to_mont(FT63, [0])
    assert np.array_equal(pos.evaluate_field_polynomial_at_point(c, zero).reshape(-1), c[:1])  # x^0 = 1 at x = 0


def test_eval_poly_equals_the_old_composition(pos, oracle):
    """lcpc_pos_side_vectors + field_dot, what the wrapper was before, at n = 1000: the same words."""
    n, d = 1000, 37
    c = oracle.random_coeffs(FT63, n, 21)
    x = oracle.ChaCha(seed_u64=5).field_random(FT63, 1)
    _, right = pos.form_side_vectors_for_polynomial_evaluation_from_point(x, 1, n)
    v = pos.field_dot(c, right)
    assert np.array_equal(pos.evaluate_field_polynomial_at_point(c, x), v)
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(x, 2, d)
    assert np.array_equal(pos.evaluate_field_polynomial_at_point_with_elevated_degree(c, x, d),
                          pos.field_dot(v, left[1]))


def _byte_sizes(T):
    tile = 7 * T
    return sorted(set(range(1, 9)) | {b + k for b in (56, tile) for k in range(-7, 8)} | {2 * tile + 57})


def test_eval_poly_bytes_host(pos, oracle):
    """n_bytes = 0..6 mod 7 around one run and one tile, tile +- 1 byte, from an odd host address."""
    rng = np.random.default_rng(4)
    x = oracle.ChaCha(seed_u64=8).field_random(FT63, 1)
    xv = oracle.from_mont(FT63, x)[0]
    buf = rng.integers(0, 256, 1 + 2 * 7 * pos.EVAL_POLY_TILE + 64, dtype=np.uint8)
    for n in _byte_sizes(pos.EVAL_POLY_TILE):
        for d in (0, (1 << 32) + 5):
            view = buf[1:1 + n]
            assert view.ctypes.data & 1
            got = pos.evaluate_bytes_polynomial_at_point(view, x, d)
            assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(view.tobytes(), xv, d), (n, d)
    assert not pos.evaluate_bytes_polynomial_at_point(b"", x, 0).any()


@pytest.mark.parametrize("off", [0, 8])
def test_eval_poly_bytes_device(pos, oracle, hipmem, native, off):
    """The device entry on a 16-byte aligned image (LDS-staged tiles) and on one only 8-byte aligned."""
    rng = np.random.default_rng(6 + off)
    x = oracle.ChaCha(seed_u64=9).field_random(FT63, 1)
    xv = oracle.from_mont(FT63, x)[0]
    sizes = _byte_sizes(pos.EVAL_POLY_TILE)
    buf = rng.integers(0, 256, off + sizes[-1] + 16, dtype=np.uint8)
    dev = hipmem.to_device(buf)
    out = np.zeros(1, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    try:
        for n in sizes:
            assert native.lcpc_pos_eval_poly_bytes_device(dev + off, n, x.ctypes.data_as(u64p), 5,
                                                          out.ctypes.data_as(u64p)) == 0
            assert oracle.from_mont(FT63, out)[0] == R.file_value(buf[off:off + n].tobytes(), xv, 5), n
        assert native.lcpc_pos_eval_poly_bytes_device(dev + 1, 56, x.ctypes.data_as(u64p), 0,
                                                      out.ctypes.data_as(u64p)) == INVALID_ARG
    finally:
        hipmem.free(dev)


def test_eval_poly_bytes_host_crosses_a_staging_block(pos, oracle):
    rng = np.random.default_rng(12)
    data = rng.integers(0, 256, pos.EVAL_STAGE_BYTES + 7 * pos.EVAL_POLY_TILE + 3, dtype=np.uint8).tobytes()
    x = oracle.ChaCha(seed_u64=10).field_random(FT63, 1)
    xv = oracle.from_mont(FT63, x)[0]
    d = (1 << 64) - 1
    got = pos.evaluate_bytes_polynomial_at_point(data, x, d)
    assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(data, xv, d)


def test_eval_poly_bytes_every_reduction_level(pos, oracle, hipmem, native):
    """7 (T^2 + 1) bytes: T^2 + 1 coefficients, so the partials reduce through three launches."""
    T = pos.EVAL_POLY_TILE
    n = 7 * (T * T + 1)
    data = np.random.default_rng(13).integers(0, 256, n, dtype=np.uint8)
    x = oracle.ChaCha(seed_u64=11).field_random(FT63, 1)
    xv = oracle.from_mont(FT63, x)[0]
    dev = hipmem.to_device(data)
    out = np.zeros(1, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    try:
        assert native.lcpc_pos_eval_poly_bytes_device(dev, n, x.ctypes.data_as(u64p), 1,
                                                      out.ctypes.data_as(u64p)) == 0
    finally:
        hipmem.free(dev)
    assert oracle.from_mont(FT63, out)[0] == R.file_value(data.tobytes(), xv, 1)


# ---------------------------------------------------------------- left multiply
def _left_case(pos, oracle, data: bytes, pre: int, seed: int):
    el = oracle.pos_bytes_to_field(data)
    n_rows = -(-el.size // pre)
    m = np.zeros(n_rows * pre, np.uint64)
    m[:el.size] = el
    left = oracle.random_coeffs(FT63, n_rows, seed)
    got = pos.left_multiply_unencoded_matrix_by_vector(data, pre, left)
    assert np.array_equal(np.asarray(got).reshape(-1), oracle.collapse(FT63, m, left, n_rows, pre)), (pre, n_rows)
    return left


@pytest.mark.parametrize("pre", [8, 64, 16384])
@pytest.mark.parametrize("rows", [1, 2, 37])
def test_left_multiply_bytes(pos, oracle, pre, rows):
    """Whole rows, a ragged last row, and a last row of one byte, against the oracle's collapse over
    the packed matrix."""
    rng = np.random.default_rng(pre + rows)
    rb = 7 * pre
    for n in (rows * rb, rows * rb - 11, (rows - 1) * rb + 1):
        _left_case(pos, oracle, rng.integers(0, 256, n, dtype=np.uint8).tobytes(), pre, n)


def test_left_multiply_bytes_pack_first_and_rejects(pos, oracle, hipmem, native):
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 7 * 4 * 9 + 5, dtype=np.uint8)
    _left_case(pos, oracle, data.tobytes(), 4, 1)       # pre = 4: packs, then the existing collapse
    _left_case(pos, oracle, data.tobytes(), 12, 2)      # not a power of two: the same path
    u64p = C.POINTER(C.c_uint64)
    n_rows = -(-(-(-data.size // 7)) // 8)
    left = oracle.random_coeffs(FT63, n_rows + 1, 4)
    out = np.zeros(8, np.uint64)
    for n_left in (n_rows - 1, n_rows + 1):
        assert native.lcpc_pos_left_multiply_bytes(data.ctypes.data, data.size, 8, left.ctypes.data_as(u64p), n_left,
                                                   out.ctypes.data_as(u64p)) == INVALID_ARG
    # the device entry, from an image that is only 8-byte aligned
    dev = hipmem.to_device(np.concatenate([np.zeros(8, np.uint8), data]))
    try:
        assert native.lcpc_pos_left_multiply_bytes_device(dev + 8, data.size, 8, left.ctypes.data_as(u64p), n_rows,
                                                          out.ctypes.data_as(u64p)) == 0
    finally:
        hipmem.free(dev)
    want = pos.left_multiply_unencoded_matrix_by_vector(data.tobytes(), 8, left[:n_rows])
    assert np.array_equal(out, want.reshape(-1))
