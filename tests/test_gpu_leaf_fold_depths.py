"""GPU: the BLAKE3 chunk-tree folds of a column leaf at the chunk counts their launchers dispatch on,
from given chaining values and from elements.  Every comparison is exact and no reference is a device
path: the folds over given chaining values are compared with read_ref.subtree_cv (pure Python), the
leaves from elements with the C oracle (oracle.hash_columns), one column per shape of which is also
pyref.blake3 of the spelled-out message.

Dispatch sites reached, and the chunk counts at which they are reached:

* blake3.hip launch_leaf_merge (lcpc_leaves_from_cvs, and behind gpu.hash_columns /
  pos.hash_columns_to_digests): k_leaf_merge alone for 2..16 chunks (one serial fold), and
  k_leaf_merge_groups + k_leaf_merge from 17 chunks on -- every count 1..65, then 127, 128, 129, 255,
  256, 257, 258, 511, 512, 513 from chaining values; 2, 3, 4, 5, 7, 8, 9, 16, 17, 18, 25 chunks from the
  elements of all five fields, row-major (k_leaf_chunks, k_leaf_chunks_words for Ft191) and
  column-major (k_leaf_chunks_cm and its two-chunk fused form, k_leaf_chunks with strides when a column
  is not 16-byte aligned); 255, 256, 256, 257 and 313 chunks (32, 33 and 40 merge groups, at 257 a last
  group of one chunk) from Ft63 elements.
* blake3.hip leaves_fold_cvs (lcpc_leaves_fold_cvs): k_leaf_fold_stack<8> for 2..256 chunks -- every
  count 2..65, 127, 128, 129, 255 and 256, where all eight levels are occupied -- and
  k_leaf_fold_stack<20> at 257, 258, 511, 512, 513.
"""
import functools

import numpy as np
import pytest

import digest_ref as R
import pyref
import read_ref

pytestmark = pytest.mark.gpu

SMALL_COUNTS = list(range(1, 66))
LARGE_COUNTS = [127, 128, 129, 255, 256, 257, 258, 511, 512, 513]
REF_COLS = (0, 63, 64)      # the first column, the last lane of the full wave, the lone lane of the partial wave
# Ft63 leaves of 255 full chunks, 256 chunks with one element in the last, 256 full chunks, 257 chunks
# with a one-block last chunk, and 313 chunks
DEEP_ROWS = (32636, 32637, 32764, 32765, 40000)
CHUNK_COUNTS = (2, 3, 4, 5, 7, 8, 9, 16, 17, 18, 25)
LEAF_COLS = (1, 65, 257)
FIELDS = [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def N(gpu):
    from lcpc_proof_of_storage_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


# ---------------------------------------------------------------- folds over given chaining values
def _cv_words(cv_bytes):
    return [int(x) for x in np.frombuffer(bytes(cv_bytes), "<u4")]


def _check_folds(N, n_chunks, n_cols, seed):
    lib = N.load()
    rng = np.random.default_rng(seed)
    cvs = rng.integers(0, 256, (n_chunks, n_cols, 32), dtype=np.uint8)
    keep = cvs.copy()
    merged = np.zeros((n_cols, 32), np.uint8)
    assert lib.lcpc_leaves_from_cvs(cvs.ctypes.data_as(N.u8p), n_chunks, n_cols, merged.ctypes.data_as(N.u8p)) == 0
    assert np.array_equal(cvs, keep), n_chunks
    folded = np.zeros((n_cols, 32), np.uint8)
    after = np.zeros_like(cvs)
    assert lib.lcpc_leaves_fold_cvs(cvs.ctypes.data_as(N.u8p), n_chunks, n_cols, folded.ctypes.data_as(N.u8p),
                                    after.ctypes.data_as(N.u8p)) == 0
    assert np.array_equal(after, keep) and np.array_equal(cvs, keep), n_chunks
    at = (n_chunks, n_cols)
    for c in REF_COLS:
        if c >= n_cols:
            continue
        column = [_cv_words(keep[i, c]) for i in range(n_chunks)]
        want = keep[0, c].tobytes()             # one chunk: the leaf is the chaining value itself
        if n_chunks > 1:
            want = read_ref._words(read_ref.subtree_cv(column, 0, n_chunks, root=True))
        assert folded[c].tobytes() == want, at + (c, "lcpc_leaves_fold_cvs")
        assert merged[c].tobytes() == want, at + (c, "lcpc_leaves_from_cvs")
    assert np.array_equal(folded, merged), at
    assert len({leaf.tobytes() for leaf in folded}) == n_cols, at


@pytest.mark.parametrize("n_cols", [1, 65])
def test_folds_of_1_to_65_chunks(N, n_cols):
    """lcpc_leaves_from_cvs and lcpc_leaves_fold_cvs over random chaining values, every chunk count 1..65.
    Columns 0, 63 and 64 (REF_COLS; column 0 alone at one column) are compared with the pure-Python fold
    read_ref.subtree_cv; the other columns must be equal between the two entries and all columns pairwise
    distinct (the inputs are, so a fold that reads a neighbour's slot shows).  Both leave their input."""
    for n_chunks in SMALL_COUNTS:
        _check_folds(N, n_chunks, n_cols, 1000 * n_cols + n_chunks)


@pytest.mark.parametrize("n_chunks", LARGE_COUNTS)
def test_folds_around_the_stack_thresholds(N, n_chunks):
    """The same at 65 columns for 127..129, 255..258 and 511..513 chunks: k_leaf_fold_stack<8> with every
    level occupied (256), the first shapes of k_leaf_fold_stack<20> (257, 258), 16 to 65 merge groups.
    Reference columns: 0, 63 and 64 (REF_COLS)."""
    _check_folds(N, n_chunks, 65, n_chunks)


# ---------------------------------------------------------------- leaves from elements
def _random_elements(fid, n_rows, n_cols, seed):
    """(n_rows, n_cols, limbs) Montgomery limbs of values below p -- random, with the residues 0 and p - 1
    sprinkled in as test_gpu_digests.leaf_matrix does"""
    f = pyref.Field(fid)
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 64, (n_rows, n_cols, f.nl), dtype=np.uint64)
    top = f.p >> (64 * (f.nl - 1))          # a top limb below p's keeps the value below p
    m[:, :, f.nl - 1] = rng.integers(0, top, (n_rows, n_cols), dtype=np.uint64)
    k = (np.arange(n_rows)[:, None] * n_cols + np.arange(n_cols)[None, :]) % 11
    m[k == 0] = np.array(R.mont_limbs(fid, 0), np.uint64)
    m[k == 5] = np.array(R.mont_limbs(fid, f.p - 1), np.uint64)
    return m


def _leaf_chunks(eb, n_rows):
    return max(1, -(-(32 + eb * n_rows) // 1024))


def leaf_rows(fid, n_chunks):
    """The row counts at which a leaf of this field has n_chunks chunks and its last chunk is exactly full
    (where the element size allows it), holds one element (Ft191: an element's tail), or ends mid-block."""
    eb = 8 * pyref.Field(fid).nl
    out = []
    if (1024 * n_chunks - 32) % eb == 0:
        out.append((1024 * n_chunks - 32) // eb)
    one = (1024 * (n_chunks - 1) - 32) // eb + 1
    out.append(one)
    mid = one
    while (32 + eb * mid - 1024 * (n_chunks - 1)) % 64 == 0 or 32 + eb * mid - 1024 * (n_chunks - 1) < 320:
        mid += 1
    out.append(mid)
    assert all(_leaf_chunks(eb, r) == n_chunks for r in out), (fid, n_chunks, out)
    last = [32 + eb * r - 1024 * (n_chunks - 1) for r in out]
    assert 0 < last[-2] <= eb and last[-1] % 64 and (len(out) == 2 or last[0] == 1024)
    return sorted(set(out))


def test_leaf_rows_are_the_stated_fills():
    """the exact fills the shapes rest on: 128 n - 4 (Ft63), 64 n - 2 (Ft127), 32 n - 1 (Ft253 / Ft255), and
    for Ft191 only at n = 2 mod 3 (84 rows for 2 chunks)"""
    for n in CHUNK_COUNTS:
        assert 128 * n - 4 in leaf_rows(0, n) and 64 * n - 2 in leaf_rows(1, n)
        assert 32 * n - 1 in leaf_rows(3, n) and 32 * n - 1 in leaf_rows(4, n)
        assert len(leaf_rows(2, n)) == (3 if n % 3 == 2 else 2)
    assert 84 in leaf_rows(2, 2)


@functools.lru_cache(maxsize=None)
def _matrix(fid):
    rows = max(r for n in CHUNK_COUNTS for r in leaf_rows(fid, n))
    return _random_elements(fid, rows, max(LEAF_COLS), 2000 + fid)


def _check_leaves(gpu, pos, oracle, fid, m, n_rows, n_cols):
    """both layouts of m's top-left corner against the oracle, the last column against pyref.blake3"""
    sub = np.ascontiguousarray(m[:n_rows, :n_cols])
    want = oracle.hash_columns(fid, sub.reshape(-1), n_rows, n_cols)
    at = (fid, n_rows, n_cols)
    c = n_cols - 1
    assert want[32 * c:32 * c + 32] == pyref.blake3(bytes(32) + R.column_bytes(fid, sub[:, c])), at
    assert gpu.hash_columns(fid, sub, n_rows, n_cols) == want, at + ("row-major",)
    cols = list(np.ascontiguousarray(sub.transpose(1, 0, 2)))
    assert b"".join(pos.hash_columns_to_digests(cols, fid)) == want, at + ("column-major",)


@pytest.mark.parametrize("n_cols", LEAF_COLS)
@pytest.mark.parametrize("fid", FIELDS)
def test_leaves_from_elements(gpu, pos, oracle, fid, n_cols):
    """gpu.hash_columns (row-major) and pos.hash_columns_to_digests (column-major) of leaves of 2, 3, 4, 5,
    7, 8, 9, 16, 17, 18 and 25 chunks, the last chunk full, holding one element and ending mid-block, at 1,
    65 and 257 columns, against oracle.hash_columns; the last column of every shape also against
    pyref.blake3 of 32 zero bytes and the column's repr bytes."""
    m = _matrix(fid)
    for n_chunks in CHUNK_COUNTS:
        for n_rows in leaf_rows(fid, n_chunks):
            _check_leaves(gpu, pos, oracle, fid, m, n_rows, n_cols)


def test_ft63_leaves_at_deep_rows(gpu, pos, oracle):
    """Ft63 leaves of DEEP_ROWS rows (255, 256, 256, 257 and 313 chunks: 32 to 40 merge groups, at 257 a
    last group of one chunk) at 65 columns, both layouts against the oracle; column 64 of every shape
    against pyref.blake3 (five columns of pure-Python BLAKE3)."""
    m = _random_elements(0, max(DEEP_ROWS), 65, 63)
    assert [_leaf_chunks(8, r) for r in DEEP_ROWS] == [255, 256, 256, 257, 313]
    for n_rows in DEEP_ROWS:
        _check_leaves(gpu, pos, oracle, 0, m, n_rows, 65)
