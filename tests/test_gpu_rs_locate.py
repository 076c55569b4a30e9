"""GPU: Reed-Solomon error location and errors-and-erasures decoding of element rows
(lcpc_rs_locate_errors_rows, lcpc_rs_decode_rows; pos.locate_errors_rows, pos.decode_rows; no
counterpart in the reference).

Rows are the oracle's fft_io codewords.  A wrong position holds a different, fully reduced seeded
random element (every seventh dirty row, if within the radius: the codeword's value + 1 -- beyond
it, + 1 at every position of a short row is another codeword), an erased position all-ones limbs
(never read).  N = len - n_per_row - n_erased syndromes per row.

* all five fields, (n_per_row, len) in {(1,2), (2,4), (3,8), (5,16), (16,32), (16,64), (512,1024)};
  1, 3 and 130 rows; n_erased in {0, 1, (len - n_per_row) / 2, len - n_per_row - 2, len - n_per_row};
* per row t wrong positions, t cycling through {0, 1, 2, N/2 - 1, N/2, N/2 + 1} -- at (512,1024) also
  63, 64, 65, 255, 256 (the wave boundaries and the smallest cap) -- so that clean rows sit between
  dirty rows of different t; positions cycling through: the first available ({0}), the last
  ({len - 1}), a contiguous run, a seeded random set;
* row_status, row_n_errors, err_mask and col_any equal the outcome of the Python reference
  (rs_locate_ref.py) for every row where len <= 64; at (512,1024), where the reference takes about
  0.1 s per dirty row, for the first three rows of every batch, and for all rows the injected sets
  (within the radius the reference's outcome IS the injected set: tests/test_rs_locate.py);
* rows is unchanged by locate; decode_rows of the batch without its t = N/2 + 1 rows gives back the
  oracle's codewords limb for limb; the batch with them returns LCPC_ERR_UNRECOVERABLE, rows unchanged;
* three rows of (16,32) with 8 wrong positions each, pairwise disjoint (their union of 24 is more
  than the 16 one erasure decode takes): still decoded;
* Ft63 at (2^14, 2^15), 3 rows: t in {1, 64, 65, 300} against the injected sets, and one row with
  lcpc_rs_locate_max_errors(FT63) + 1 wrong positions: status 2 by the cap.
"""
import numpy as np
import pytest

import rs_locate_ref as R

pytestmark = pytest.mark.gpu
FIELDS = [0, 1, 2, 3, 4]
SHAPES = [(1, 2), (2, 4), (3, 8), (5, 16), (16, 32), (16, 64), (512, 1024)]
N_ROWS = [1, 3, 130]


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos
    return pos


def erasure_counts(npr, length):
    m = length - npr
    return sorted({0, 1, m // 2, max(m - 2, 0), m} & set(range(m + 1)))


def t_values(npr, length, n_erased):
    N = length - npr - n_erased
    ts = {0, 1, 2, N // 2 - 1, N // 2, N // 2 + 1}
    if length == 1024:
        ts |= {63, 64, 65, 255, 256}
    return sorted(t for t in ts if 0 <= t <= length - n_erased)


def build_batch(fid, npr, length, n_erased, seed, radius_only=False):
    """(rows, erased, expect): 130 damaged rows and per row the expected (status, n_errors, positions)
    from what was injected.  radius_only: rows beyond the radius are left clean (a decodable batch)."""
    cw = R.codewords(fid, npr, length)
    rng = np.random.default_rng(seed)
    erased = sorted(int(c) for c in rng.permutation(length)[:n_erased])
    avail = [c for c in range(length) if c not in erased]
    N = length - npr - n_erased
    ts = t_values(npr, length, n_erased)
    if N == 0 and radius_only:
        ts = [0]                                   # no syndromes: nothing wrong can be seen or mended
    # dirty rows first so that the 1- and 3-row prefixes are not all clean
    order = [t for t in ts if t] + [0] if len(ts) > 1 else ts
    rows = np.array(cw, np.uint64).copy()
    expect = []
    dirty = 0
    for r in range(130):
        t = order[r % len(order)]
        if radius_only and 2 * t > N:
            t = 0
        where = R.error_positions(avail, t, (r // len(order)) % 4, rng)
        rows[r] = R.damage(fid, cw[r], where, erased, rng, plus_one=(0 < 2 * t <= N and dirty % 7 == 3))
        dirty += t > 0
        if N == 0 or t == 0:
            expect.append((0, 0, []))
        elif 2 * t <= N:
            expect.append((1, t, sorted(where)))
        else:
            expect.append((2, 0, []))
    return rows, erased, expect


def check_locate(pos, fid, rows, npr, erased, expect):
    keep = rows.copy()
    status, n_err, mask, col_any = pos.locate_errors_rows(fid, rows, npr, erased)
    assert np.array_equal(rows, keep)
    length = rows.shape[1]
    want_any = np.zeros(length, np.uint8)
    for r, (st, L, where) in enumerate(expect):
        assert (int(status[r]), int(n_err[r])) == (st, L), (fid, npr, length, len(erased), r, expect[r])
        assert [int(c) for c in np.flatnonzero(mask[r])] == where, (fid, npr, length, len(erased), r)
        want_any[where] = 1
    assert np.array_equal(col_any, want_any)


@pytest.mark.parametrize("npr,length", SHAPES)
@pytest.mark.parametrize("fid", FIELDS)
def test_locate_and_decode(pos, oracle, fid, npr, length):
    from lcpc_proof_of_storage_amd import lcpc2d
    cw = R.codewords(fid, npr, length)
    for n_erased in erasure_counts(npr, length):
        seed = 77000 + 1000 * fid + length + 7 * n_erased
        rows, erased, expect = build_batch(fid, npr, length, n_erased, seed)
        # the reference's outcome: every row of the short shapes, the first three rows at (512, 1024)
        loc = R.Locator(pos, fid, length, npr, erased, max_errors=pos.rs_locate_max_errors(fid))
        for r in range(130 if length <= 64 else 3):
            assert loc.locate(rows[r]) == expect[r], (fid, npr, length, n_erased, r)
        for n_rows in N_ROWS:
            check_locate(pos, fid, rows[:n_rows], npr, erased, expect[:n_rows])
        # a row beyond the radius: nothing is decoded, nothing written
        bad = [r for r, e in enumerate(expect) if e[0] == 2]
        if bad:
            n = bad[0] + 1
            with pytest.raises(lcpc2d.DeviceError) as e:
                pos.decode_rows(fid, rows[:n], npr, erased)
            assert e.value.code == pos.UNRECOVERABLE
        ok_rows, erased2, ok_expect = build_batch(fid, npr, length, n_erased, seed, radius_only=True)
        assert erased2 == erased and all(e[0] != 2 for e in ok_expect)
        for n_rows in N_ROWS:
            got = pos.decode_rows(fid, ok_rows[:n_rows], npr, erased)
            assert np.array_equal(got, cw[:n_rows]), (fid, npr, length, n_erased, n_rows)


@pytest.mark.parametrize("fid", FIELDS)
def test_unrecoverable_batch_is_left_unchanged(pos, oracle, fid):
    """the C entry: one status-2 row among located ones -> LCPC_ERR_UNRECOVERABLE, row_status filled,
    every row (the all-ones erased positions included) unchanged"""
    from lcpc_proof_of_storage_amd import _native as N
    npr, length = 16, 32
    rows, erased, expect = build_batch(fid, npr, length, 1, 4242 + fid)
    rows = np.ascontiguousarray(rows[:12])
    assert {e[0] for e in expect[:12]} == {0, 1, 2}
    keep = rows.copy()
    status = np.zeros(12, np.uint8)
    e = np.asarray(erased, np.uint64)
    rc = N.load().lcpc_rs_decode_rows(fid, rows.ctypes.data_as(N.u64p), 12, length, npr, e.ctypes.data_as(N.u64p),
                                      e.size, status.ctypes.data_as(N.u8p))
    assert rc == 36
    assert np.array_equal(rows, keep)
    assert [int(s) for s in status] == [x[0] for x in expect[:12]]


@pytest.mark.parametrize("fid", FIELDS)
def test_disjoint_error_sets_split_into_groups(pos, oracle, fid):
    npr, length = 16, 32
    cw = R.codewords(fid, npr, length)[:3]
    rng = np.random.default_rng(99 + fid)
    perm = [int(c) for c in rng.permutation(length)]
    rows = np.array(cw, np.uint64).copy()
    sets = [sorted(perm[8 * r:8 * r + 8]) for r in range(3)]
    for r in range(3):
        rows[r] = R.damage(fid, cw[r], sets[r], [], rng)
    status, n_err, mask, _ = pos.locate_errors_rows(fid, rows, npr)
    assert [int(s) for s in status] == [1, 1, 1] and [int(x) for x in n_err] == [8, 8, 8]
    assert [[int(c) for c in np.flatnonzero(mask[r])] for r in range(3)] == sets
    assert np.array_equal(pos.decode_rows(fid, rows, npr), cw)


def test_single_row_without_row_axis(pos, oracle):
    cw = R.codewords(1, 5, 16)[0]
    rng = np.random.default_rng(5)
    row = R.damage(1, cw, [4, 11], [2, 9, 15], rng)
    assert np.array_equal(pos.decode_rows(1, row, 5, [15, 2, 9]), cw)


def test_file_default_shape_ft63(pos, oracle):
    """(2^14, 2^15): N = 2^14 syndromes.  The Python reference is too slow here; the expectations are
    the injected sets."""
    fid, npr, length = 0, 1 << 14, 1 << 15
    cw = R.codewords(fid, npr, length, 3)
    rng = np.random.default_rng(2024)
    cap = pos.rs_locate_max_errors(fid)
    assert 300 <= cap < 8192
    avail = list(range(length))
    for ts in ([1, 64, 65], [300, 0, 1], [1, cap + 1, 64]):
        rows = np.array(cw, np.uint64).copy()
        sets = []
        for r, t in enumerate(ts):
            where = R.error_positions(avail, t, 3 if t > 1 else r % 2, rng)
            rows[r] = R.damage(fid, cw[r], where, [], rng)
            sets.append(where)
        status, n_err, mask, col_any = pos.locate_errors_rows(fid, rows, npr)
        for r, t in enumerate(ts):
            if t > cap:
                assert (int(status[r]), int(n_err[r])) == (2, 0) and not mask[r].any()
                continue
            assert (int(status[r]), int(n_err[r])) == (1 if t else 0, t), (ts, r)
            assert [int(c) for c in np.flatnonzero(mask[r])] == sets[r], (ts, r)
        if max(ts) <= cap:
            assert np.array_equal(pos.decode_rows(fid, rows, npr), cw)
