"""GPU: Reed-Solomon erasure decoding of element rows (lcpc_rs_erasure_decode_rows, pos.erasure_decode_rows;
no counterpart in the reference).

Rows are the oracle's fft_io codewords of random messages of n_per_row coefficients.  The erased
positions are overwritten with all-ones limbs (not a canonical element: the call must never read
them) and the call must give back the oracle's codeword limb for limb -- every recovered value
fully reduced, every other limb untouched.

* all five fields, (n_per_row, len) in {(1,2), (3,8), (5,16), (16,32), (512,1024)}; Ft63 also at
  (2^14, 2^15), the stored files' default shape (the one-pass and four-step transforms, and three
  row batches at 130 rows);
* 1, 3 and 130 rows;
* erasure sets: empty, {0}, {len-1}, a contiguous run of len - n_per_row, a seeded random set of
  len - n_per_row, a random set of half that size;
* len - n_per_row + 1 erasures: LCPC_ERR_UNRECOVERABLE; a duplicate or out-of-range index:
  LCPC_ERR_INVALID_ARG; fewer than the maximum erasures plus one corrupted surviving element:
  LCPC_ERR_UNRECOVERABLE with the rows unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIELDS = [0, 1, 2, 3, 4]
SHAPES = [(1, 2), (3, 8), (5, 16), (16, 32), (512, 1024)]
N_ROWS = [1, 3, 130]
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_codewords = {}


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos
    return pos


def codewords(oracle, fid, npr, length):
    """130 codewords (130, len, limbs) of seeded random messages, computed once per shape; never modified."""
    key = (fid, npr, length)
    if key not in _codewords:
        nl = oracle.limbs(fid)
        msgs = oracle.random_coeffs(fid, 130 * npr, 0xE5A5 + 131 * fid + length).reshape(130, npr * nl)
        rows = np.zeros((130, length * nl), np.uint64)
        for r in range(130):
            row = np.zeros(length * nl, np.uint64)
            row[:npr * nl] = msgs[r]
            rows[r] = oracle.fft_io(fid, row)
        rows = rows.reshape(130, length, nl)
        rows.setflags(write=False)
        _codewords[key] = rows
    return _codewords[key]


def erasure_sets(npr, length):
    m = length - npr
    rng = np.random.default_rng(1000 * length + npr)
    sets = [[], [0], [length - 1], list(range(npr // 2, npr // 2 + m)),
            [int(c) for c in rng.permutation(length)[:m]],
            [int(c) for c in rng.permutation(length)[:m // 2]]]
    return sets


def _check_shape(pos, oracle, fid, npr, length):
    want_all = codewords(oracle, fid, npr, length)
    for n_rows in N_ROWS:
        want = want_all[:n_rows]
        for erased in erasure_sets(npr, length):
            damaged = want.copy()
            damaged[:, erased, :] = ONES
            got = pos.erasure_decode_rows(fid, damaged, npr, erased)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (fid, npr, length, n_rows, len(erased))


@pytest.mark.parametrize("npr,length", SHAPES)
@pytest.mark.parametrize("fid", FIELDS)
def test_erased_positions_are_recovered_limb_for_limb(pos, oracle, fid, npr, length):
    _check_shape(pos, oracle, fid, npr, length)


def test_file_default_shape_ft63(pos, oracle):
    """(2^14, 2^15): the PoS default dims; 130 rows go through the device in three batches"""
    _check_shape(pos, oracle, 0, 1 << 14, 1 << 15)


def test_single_row_without_row_axis(pos, oracle):
    want = codewords(oracle, 1, 5, 16)[0]
    damaged = want.copy()
    damaged[[2, 9, 15]] = ONES
    assert np.array_equal(pos.erasure_decode_rows(1, damaged, 5, [15, 2, 9]), want)


@pytest.mark.parametrize("npr,length", [(1, 2), (5, 16), (512, 1024)])
@pytest.mark.parametrize("fid", FIELDS)
def test_error_cases(pos, oracle, fid, npr, length):
    from lcpc_proof_of_storage_amd import _native as N
    from lcpc_proof_of_storage_amd import lcpc2d
    lib = N.load()
    want = codewords(oracle, fid, npr, length)[:3]
    m = length - npr

    def call(rows, erased, n_per_row=npr):
        e = np.asarray(erased, np.uint64)
        return lib.lcpc_rs_erasure_decode_rows(fid, rows.ctypes.data_as(N.u64p), rows.shape[0], length, n_per_row,
                                               e.ctypes.data_as(N.u64p) if e.size else None, e.size)
    rows = want.copy()
    assert call(rows, list(range(m + 1))) == 36                 # LCPC_ERR_UNRECOVERABLE
    assert call(rows, [0, 0]) == 30                             # LCPC_ERR_INVALID_ARG
    assert call(rows, [length]) == 30
    assert call(rows, [], 0) == 30 and call(rows, [], length) == 30
    assert np.array_equal(rows, want)
    # fewer than the maximum erasures and one corrupted surviving element: the degree check sees it
    for n_erased in sorted({0, m // 2, m - 1}):
        erased = list(range(1, 1 + n_erased))
        rows = want.copy()
        rows[:, erased, :] = ONES
        rows[1, 0, 0] ^= np.uint64(1 << 7)                      # row 1, position 0 (never erased here)
        keep = rows.copy()
        assert call(rows, erased) == 36, n_erased
        assert np.array_equal(rows, keep), n_erased
        with pytest.raises(lcpc2d.DeviceError) as e:
            pos.erasure_decode_rows(fid, keep, npr, erased)
        assert e.value.code == pos.UNRECOVERABLE
    # the same rows without the corruption pass the check (n_erased == 0 is the check alone)
    assert call(want.copy(), []) == 0
