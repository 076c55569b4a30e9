"""GPU: checkable reads end to end (FileHandler.read_rows_response / read_opening_response ->
pos.client_verify_read): every kind of chunk range is accepted and returns the file's bytes, the
rebuilt leaves are the tree's, the covers are the pure-Python reference's, the cached and uncached
servers answer with the same bytes, the opening has the stated size, reads follow edits and appends,
and every forged answer is rejected with its kind.  All comparisons are exact."""
import copy

import numpy as np
import pytest

import read_ref as R

pytestmark = pytest.mark.gpu
FT63 = 0
UNSUPPORTED = 34
DIMS = [(8, 16), (64, 128)]
# one chunk (ROOT on the chunk); two chunks; three, left-balanced; a ragged last chunk; 19 chunks
# (three merge groups, the last one short) and 36 (five groups: not a power of two)
ROWS = [1, 124, 125, 253, 700, 1149, 2400, 4500]


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _handler(PF, directory, name, data, pre, enc, chunk_cache):
    src = directory / f"{name}.bin"
    src.write_bytes(data)
    return PF.FileHandler.create_from_unencoded_file("01READ" + "0" * 20, str(src), pre, enc,
                                                     directory=str(directory / name), chunk_cache=chunk_cache)


@pytest.fixture(scope="module")
def stored(PF, tmp_path_factory):
    """(pre, enc, rows) -> (contents, handler without a cache, handler with one), made once."""
    made = {}

    def get(pre, enc, rows):
        key = (pre, enc, rows)
        if key not in made:
            d = tmp_path_factory.mktemp(f"read_{pre}_{enc}_{rows}")
            data = _bytes(rows * 7 * pre - 3, rows + enc)    # a ragged last row
            made[key] = (data, _handler(PF, d, "plain", data, pre, enc, False),
                         _handler(PF, d, "cached", data, pre, enc, True))
        return made[key]

    return get


def _ranges(file_len, pre, rows):
    """Byte ranges whose rows lie in the first chunk only, the last only, a middle one, across the
    tree's top split, and the whole file."""
    rb = 7 * pre
    n = R.n_chunks(rows)
    out = [(3, min(5 * rb, file_len)), ((rows - 1) * rb + 1, file_len), (0, file_len)]
    if n >= 3:
        r = R.chunk_first_row(n // 2) + 1
        out.append((r * rb + 2, (r + 2) * rb))            # ends on a row boundary
    if n >= 2:
        split = 1
        while 2 * split < n:
            split *= 2
        r = R.chunk_first_row(split)
        out.append(((r - 1) * rb + 2, (r + 1) * rb - 1))
    return sorted({(a, b) for a, b in out if 0 <= a < b <= file_len})


def _columns(enc, k, seed):
    return sorted(int(c) for c in np.random.default_rng(seed).choice(enc, size=min(k, enc), replace=False))


def _same(a, b):
    return (np.array_equal(a.segments, b.segments) and np.array_equal(a.covers, b.covers)
            and [list(p) for p in a.paths] == [list(p) for p in b.paths])


@pytest.mark.parametrize("pre,enc", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_reads_verify(pos, stored, pre, enc, rows):
    data, plain, cached = stored(pre, enc, rows)
    root = plain.get_commit_root()
    assert cached.get_commit_root() == root and cached.chunk_cache is not None and plain.chunk_cache is None
    cols = _columns(enc, 11, rows)
    path_len = enc.bit_length() - 1
    ref_cols = {c: [int(v) for v in np.asarray(plain.read_full_columns([c])[0].col).reshape(-1)] for c in cols[:2]}
    ref_cvs = {c: R.column_chunk_cvs(v) for c, v in ref_cols.items()}
    for c, v in ref_cols.items():
        assert R.leaf(v) == plain.get_merkle_tree()[c]
    for a, b in _ranges(len(data), pre, rows):
        plan = pos.read_plan(len(data), a, b, pre)
        rows_msg = plain.read_rows_response(a, b)
        assert rows_msg == cached.read_rows_response(a, b)
        assert rows_msg == data[plan.row_lo * 7 * pre:min(plan.row_hi * 7 * pre, len(data))]
        opening = plain.read_opening_response(a, b, cols)
        assert _same(opening, cached.read_opening_response(a, b, cols)), (a, b)
        seg_rows = plan.seg_row_hi - plan.seg_row_lo
        assert opening.n_bytes() == len(cols) * (8 * seg_rows + 32 * plan.n_cover + 32 * path_len)
        assert opening.segments.shape == (len(cols), seg_rows)
        assert pos.client_verify_read(root, len(data), pre, enc, a, b, rows_msg, cols, opening, seed=a + 1) == data[a:b]
        leaves, dots, ok = pos.segment_leaves(opening.segments, rows, plan.chunk_lo, plan.chunk_hi, opening.covers)
        assert dots is None and ok.all()
        assert [leaves[k].tobytes() for k in range(len(cols))] == [plain.get_merkle_tree()[c] for c in cols], (a, b)
        for k, c in enumerate(cols[:2]):
            want = [R._words(R.subtree_cv(ref_cvs[c], lo, hi)) for lo, hi in plan.cover_nodes]
            assert [opening.covers[k, j].tobytes() for j in range(plan.n_cover)] == want, (a, b, c)
            assert [int(v) for v in opening.segments[k]] == ref_cols[c][plan.seg_row_lo:plan.seg_row_hi]
    # a read with the client's own randomness (no seed) passes as well
    a, b = _ranges(len(data), pre, rows)[-1]
    opening = cached.read_opening_response(a, b, cols)
    assert pos.client_verify_read(root, len(data), pre, enc, a, b, cached.read_rows_response(a, b), cols,
                                  opening) == data[a:b]


@pytest.mark.parametrize("rows", [125, 1149, 4500])
def test_weighted_sums_equal_integer_sums(pos, stored, rows):
    pre, enc = 64, 128
    data, plain, _ = stored(pre, enc, rows)
    cols = _columns(enc, 7, 3)
    a, b = 0, len(data)
    plan = pos.read_plan(len(data), a, b, pre)
    opening = plain.read_opening_response(a, b, cols)
    w = np.random.default_rng(rows).integers(0, R.P, plan.seg_row_hi - plan.seg_row_lo, dtype=np.uint64)
    w[::5] = 0
    leaves, dots, ok = pos.segment_leaves(opening.segments, rows, plan.chunk_lo, plan.chunk_hi, opening.covers, w)
    assert ok.all() and [leaves[k].tobytes() for k in range(len(cols))] == [plain.get_merkle_tree()[c] for c in cols]
    wv = [R.from_mont(x) for x in w]
    for k in range(len(cols)):
        assert R.from_mont(dots[k]) == sum(u * int(e) for u, e in zip(wv, opening.segments[k])) % R.P


def test_default_dims(pos, PF, tmp_path):
    """(16384, 32768), 130 rows: two chunks, the default column count, the one-pass row encode."""
    pre, enc, rows = 16384, 32768, 130
    data = _bytes(rows * 7 * pre - 11, 7)
    fh = _handler(PF, tmp_path, "default", data, pre, enc, True)
    cols = _columns(enc, pos.get_PoS_soudness_n_cols(pre, enc), 5)
    assert len(cols) == 309
    for a, b in [(126 * 7 * pre + 5, 127 * 7 * pre + 9), (0, len(data))]:
        plan = pos.read_plan(len(data), a, b, pre)
        opening = fh.read_opening_response(a, b, cols)
        assert opening.covers.shape == (309, plan.n_cover, 32)
        got = pos.client_verify_read(fh.get_commit_root(), len(data), pre, enc, a, b, fh.read_rows_response(a, b), cols,
                                     opening, seed=2)
        assert got == data[a:b]
    assert plan.n_cover == 0 and pos.read_plan(len(data), 126 * 7 * pre, 126 * 7 * pre + 1, pre).cover_nodes == [(0, 1)]


def _rejected(pos, kind, *args):
    with pytest.raises(pos.VerifierError) as e:
        pos.client_verify_read(*args, seed=9)
    assert e.value.kind == kind, e.value


def test_forgeries_rejected(pos, stored):
    pre, enc, rows = 64, 128, 1149
    data, plain, _ = stored(pre, enc, rows)
    rb = 7 * pre
    r = R.chunk_first_row(5) + 40                       # rows inside chunk 5 of 10
    a, b = r * rb + 2, (r + 3) * rb - 1
    cols = _columns(enc, 12, 4)
    root = plain.get_commit_root()
    plan = pos.read_plan(len(data), a, b, pre)
    assert plan.n_cover >= 3 and plan.seg_row_lo < plan.row_lo and plan.row_hi < plan.seg_row_hi
    rows_msg = plain.read_rows_response(a, b)
    opening = plain.read_opening_response(a, b, cols)
    args = (root, len(data), pre, enc, a, b)
    assert pos.client_verify_read(*args, rows_msg, cols, opening, seed=9) == data[a:b]

    # one flipped byte in data (in the rows read but outside the range asked for, too)
    for at in (0, len(rows_msg) // 2, len(rows_msg) - 1):
        bad = bytearray(rows_msg)
        bad[at] ^= 0x10
        _rejected(pos, "ReadMismatch", *args, bytes(bad), cols, opening)
    _rejected(pos, "ColumnEval", *args, rows_msg[:-1], cols, opening)

    def forged(fn):
        o = copy.deepcopy(opening)
        fn(o)
        return o

    def set_seg(o, k, i, v):
        o.segments[k, i] = np.uint64(v)

    inside = plan.row_lo - plan.seg_row_lo + 1
    # a changed segment element inside the read rows, and outside them but inside the segment
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(lambda o: set_seg(o, 3, inside, int(o.segments[3, inside]) ^ 1)))
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(lambda o: set_seg(o, 0, 0, int(o.segments[0, 0]) ^ 1)))
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(lambda o: set_seg(o, 11, -1, int(o.segments[11, -1]) ^ 1)))
    # an element that is not < p
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(lambda o: set_seg(o, 2, inside, R.P)))
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(lambda o: set_seg(o, 2, 1, (1 << 64) - 1)))

    # a changed cover, two covers swapped, a cover dropped
    def flip_cover(o):
        o.covers[5, 1, 7] ^= 1

    def swap_covers(o):
        o.covers[5, [0, 1]] = o.covers[5, [1, 0]]

    def drop_cover(o):
        o.covers = np.ascontiguousarray(o.covers[:, :-1])

    assert not np.array_equal(opening.covers[5, 0], opening.covers[5, 1])
    for fn in (flip_cover, swap_covers, drop_cover):
        _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(fn))

    # a path digest changed
    def flip_path(o):
        p = o.paths[4][2]
        o.paths[4][2] = bytes([p[0] ^ 1]) + p[1:]

    _rejected(pos, "ColumnEval", *args, rows_msg, cols, forged(flip_path))
    # an opening of other columns than the ones asked for
    _rejected(pos, "ColumnEval", *args, rows_msg, cols, plain.read_opening_response(a, b, sorted(c ^ 1 for c in cols)))
    # the honest answer still passes
    assert pos.client_verify_read(*args, rows_msg, cols, opening, seed=9) == data[a:b]


@pytest.mark.parametrize("chunk_cache", [False, True])
def test_reads_follow_edits_and_appends(pos, PF, tmp_path, chunk_cache):
    pre, enc = 64, 128
    rb = 7 * pre
    data = _bytes(700 * rb - 3, 21)
    fh = _handler(PF, tmp_path, "edited", data, pre, enc, chunk_cache)
    other = _handler(PF, tmp_path, "twin", data, pre, enc, not chunk_cache)
    cols = _columns(enc, 12, 8)
    a, b = 300 * rb + 5, 302 * rb                          # rows 300 and 301, chunk 2 of 6
    steps = [("edit", 300 * rb + 100, _bytes(rb, 22)),     # inside the range read
             ("append", None, _bytes(130 * rb + 7, 23)),   # one more chunk: every cover changes shape
             ("edit", 5 * rb, _bytes(9, 24))]              # outside the segment: only a cover changes
    for what, offset, patch in steps:
        old_root, old_len = fh.get_commit_root(), fh.get_total_data_bytes()
        old_rows = fh.read_rows_response(a, b)
        old_opening = fh.read_opening_response(a, b, cols)
        for h in (fh, other):
            if what == "edit":
                h.edit_bytes(offset, patch)
            else:
                h.append_bytes(patch)
        data = data + patch if what == "append" else data[:offset] + patch + data[offset + len(patch):]
        root, n = fh.get_commit_root(), fh.get_total_data_bytes()
        assert root != old_root and n == len(data) and other.get_commit_root() == root
        rows_msg = fh.read_rows_response(a, b)
        opening = fh.read_opening_response(a, b, cols)
        assert _same(opening, other.read_opening_response(a, b, cols)), what
        assert pos.client_verify_read(root, n, pre, enc, a, b, rows_msg, cols, opening, seed=3) == data[a:b]
        # the new answer does not verify against the old root, nor the old answer against the new
        with pytest.raises(pos.VerifierError):
            pos.client_verify_read(old_root, old_len, pre, enc, a, b, rows_msg, cols, opening, seed=3)
        _rejected(pos, "ColumnEval", root, n, pre, enc, a, b, old_rows, cols, old_opening)
        if rows_msg != old_rows:
            # stale rows from before the edit with the current openings
            _rejected(pos, "ReadMismatch", root, n, pre, enc, a, b, old_rows, cols, opening)
    assert rows_msg == old_rows   # (the last edit was elsewhere)


def test_other_digest_is_unsupported(gpu, pos, stored):
    pre, enc, rows = 8, 16, 125
    data, plain, _ = stored(pre, enc, rows)
    cols = _columns(enc, 5, 1)
    a, b = 10, 40
    rows_msg, opening = plain.read_rows_response(a, b), plain.read_opening_response(a, b, cols)
    code = gpu.LigeroEncoding.new_from_dims(FT63, pre, enc)
    assert pos._verify_read(code, plain.get_commit_root(), len(data), a, b, rows_msg, cols, opening) == data[a:b]
    for d in (1, 2, 3):
        other = gpu.LigeroEncoding.new_from_dims(FT63, pre, enc).set_digest(d)
        with pytest.raises(gpu.LcpcError) as e:
            pos._verify_read(other, plain.get_commit_root(), len(data), a, b, rows_msg, cols, opening)
        assert e.value.code == UNSUPPORTED


def test_argument_errors(gpu, pos, PF, stored):
    from lcpc_proof_of_storage_amd import _native as N
    pre, enc, rows = 8, 16, 700
    data, plain, cached = stored(pre, enc, rows)
    lib = N.load()
    n = R.n_chunks(rows)
    seg = np.zeros((2, 128), np.uint64)
    cov = np.zeros((2, 4, 32), np.uint8)
    leaves, ok = np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    u8, u64 = (lambda x: x.ctypes.data_as(N.u8p)), (lambda x: x.ctypes.data_as(N.u64p))
    n_cover = len(R.cover_nodes(n, 2, 3))

    def leaves_status(chunk_lo, chunk_hi, k, weights=None, dots=None):
        return lib.lcpc_pos_segment_leaves(u64(seg), 2, rows, chunk_lo, chunk_hi, u8(cov), k, weights, u8(leaves), dots,
                                           u8(ok))

    assert leaves_status(2, 3, n_cover) == 0
    assert leaves_status(2, 3, n_cover + 1) == 30 and leaves_status(2, 3, n_cover - 1) == 30
    assert leaves_status(2, 2, n_cover) == 30 and leaves_status(3, 2, n_cover) == 30
    assert leaves_status(n - 1, n + 1, n_cover) == 30
    assert leaves_status(2, 3, n_cover, u64(np.zeros(128, np.uint64)), None) == 30
    idx = np.array([1, 5], np.uint64)
    h = cached.chunk_cache._h
    assert lib.lcpc_pos_segment_covers_from_cache(h, u64(idx), 2, 2, 2, u8(cov)) == 30
    assert lib.lcpc_pos_segment_covers_from_cache(h, u64(idx), 2, 0, n + 1, u8(cov)) == 30
    assert lib.lcpc_pos_segment_covers_from_cache(h, u64(np.array([1, enc], np.uint64)), 2, 2, 3, u8(cov)) == 30
    # the cache is the same after it was opened from
    before = cached.chunk_cache.copy_cvs()
    pos.segment_covers_from_cache(cached.chunk_cache, [0, 3, 15], 2, 3)
    assert np.array_equal(before, cached.chunk_cache.copy_cvs())
    # a non-canonical element in a whole column is an error of the server's call
    whole = np.stack([np.asarray(plain.read_full_columns([c])[0].col, dtype=np.uint64).reshape(-1) for c in (1, 5)])
    assert np.array_equal(pos.segment_covers_from_columns(whole, rows, 2, 3),
                          pos.segment_covers_from_cache(cached.chunk_cache, [1, 5], 2, 3))
    whole[1, 650] = np.uint64(R.P)
    with pytest.raises(gpu.LcpcError) as e:
        pos.segment_covers_from_columns(whole, rows, 2, 3)
    assert e.value.code == 30
