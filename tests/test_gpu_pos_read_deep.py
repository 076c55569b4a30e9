"""GPU: the column chunk-CV cache and the checkable reads of stored files whose leaves have 256 and 257
BLAKE3 chunks (32764 and 32765 rows at pre = 8, enc = 16), the two sides of the `n_chunks <= 256` test of
their folds.  The references are the C oracle's encode (oracle.pos_encode_file) and the pure-Python cover
walk (read_ref); every comparison is exact.

Dispatch sites reached, and the chunk counts at which they are reached:

* blake3.hip leaves_fold_cvs (the cache's tree): k_leaf_fold_stack<8> at 256 chunks with every level
  occupied, k_leaf_fold_stack<20> at 257, both when the cache is built and after a one-byte edit.
* pos_read.hip read_cover_values: k_cover_values<8> at 256 chunks (covers of 1 to 128 chunks),
  k_cover_values<20> at 257 (covers of 1 to 256 chunks), for the cached and the uncached server.
* pos_read.hip read_segment_leaves: k_segment_leaves<8> at 256 chunks -- with the last row read the
  program pushes eight covers and one chunk, so all eight levels of CvStack<8> and its top are occupied
  -- and k_segment_leaves<20> at 257; ranges in the first chunk, the last, across the 127 | 128 seam,
  across the 255 | 256 seam (the top split of the 257-chunk tree), over 31 chunks and over the whole
  file (the READ_OP_GROUPS form, past 16 chunks).
"""
import copy

import numpy as np
import pytest

import read_ref as R
from test_gpu_pos_read import PF, _bytes, _handler, _same, pos, stored  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu
PRE, ENC = 8, 16
RB = 7 * PRE
DEEP = (32764, 32765)          # 256 full chunks; 257 chunks, the last one one block long
COLS = [0, 6, 15]


def _ranges(rows, file_len):
    """name -> byte range: the first row only, the last row only, across rows 16379 | 16380 (chunks 127 |
    128), across rows 32763 | 32764 (chunks 255 | 256, where the file has them), rows of chunks 120 to 150,
    and the whole file"""
    out = {"first": (3, RB - 1), "last": ((rows - 1) * RB + 1, file_len),
           "seam 127|128": (16379 * RB + 2, 16381 * RB - 1),
           "31 chunks": ((R.chunk_first_row(120) + 5) * RB + 2, (R.chunk_first_row(150) + 9) * RB),
           "whole": (0, file_len)}
    if rows > 32764:
        out["seam 255|256"] = (32763 * RB + 2, min(32765 * RB - 1, file_len))
    return out


@pytest.fixture(scope="module")
def encoded(oracle, stored):
    """rows -> (contents, uncached handler, cached handler, the oracle's tree): made once"""
    made = {}

    def get(rows):
        if rows not in made:
            data, plain, cached = stored(PRE, ENC, rows)
            _, o_tree, o_rows, _ = oracle.pos_encode_file(data, PRE, ENC)
            assert o_rows == rows == plain.get_dimensions()[2] and R.n_chunks(rows) == 256 + (rows > 32764)
            made[rows] = (data, plain, cached, o_tree)
        return made[rows]

    return get


@pytest.mark.parametrize("rows", DEEP)
def test_trees_equal_the_oracles(encoded, rows):
    """both handlers' trees, and the tree folded from the cache's chaining values, are the oracle's"""
    data, plain, cached, o_tree = encoded(rows)
    assert plain.chunk_cache is None and cached.chunk_cache is not None
    assert cached.chunk_cache.n_chunks == R.n_chunks(rows)
    assert plain.get_merkle_tree().to_bytes() == o_tree
    assert cached.get_merkle_tree().to_bytes() == o_tree
    assert cached.chunk_cache.tree().to_bytes() == o_tree


@pytest.mark.parametrize("rows", DEEP)
def test_edit_in_the_last_row_through_the_cache(PF, oracle, tmp_path, rows):
    """one byte changed in the last row: the cached handler rehashes one chunk and folds all of them
    (k_leaf_fold_stack<8> at 256 chunks, <20> at 257); its tree is the oracle's and a fresh uncached
    encode's of the edited contents"""
    data = bytearray(_bytes(rows * RB - 3, rows + ENC))
    cached = _handler(PF, tmp_path, "cached", bytes(data), PRE, ENC, True)
    at = (rows - 1) * RB + 5
    new = bytes([data[at] ^ 0x40])
    old, tree = cached.edit_bytes(at, new)
    assert old == bytes(data[at:at + 1])
    data[at:at + 1] = new
    n = R.n_chunks(rows)
    assert cached.last_chunk_range == (n - 1, n)
    fresh = _handler(PF, tmp_path, "fresh", bytes(data), PRE, ENC, False)
    _, o_tree, _, _ = oracle.pos_encode_file(bytes(data), PRE, ENC)
    assert tree.to_bytes() == o_tree == fresh.get_merkle_tree().to_bytes()
    assert cached.get_merkle_tree().to_bytes() == o_tree


@pytest.mark.parametrize("rows", DEEP)
def test_reads_verify(pos, encoded, rows):
    """Every range of _ranges with three opened columns: client_verify_read accepts and returns the file's
    bytes, the cached and the uncached server answer identically, the rebuilt leaves are the oracle
    tree's.  For the first-row and the last-row range, on column 6, the covers equal read_ref's (one
    column of pure-Python chunk CVs per file) and read_ref.leaf_from_opening gives the tree's leaf; a cover
    with one bit flipped is rejected."""
    data, plain, cached, o_tree = encoded(rows)
    root = o_tree[-32:]
    assert plain.get_commit_root() == root == cached.get_commit_root()
    leaves = [o_tree[32 * c:32 * c + 32] for c in COLS]
    n = R.n_chunks(rows)
    column = [int(v) for v in np.asarray(plain.read_full_columns([COLS[1]])[0].col).reshape(-1)]
    ref_cvs = R.column_chunk_cvs(column)
    for name, (a, b) in _ranges(rows, len(data)).items():
        plan = pos.read_plan(len(data), a, b, PRE)
        want_plan = R.read_plan(len(data), a, b, PRE)
        assert (plan.chunk_lo, plan.chunk_hi, plan.n_cover) == (want_plan["chunk_lo"], want_plan["chunk_hi"],
                                                                len(want_plan["cover_nodes"])), name
        rows_msg = plain.read_rows_response(a, b)
        assert rows_msg == cached.read_rows_response(a, b)
        opening = plain.read_opening_response(a, b, COLS)
        assert _same(opening, cached.read_opening_response(a, b, COLS)), name
        assert opening.covers.shape == (len(COLS), plan.n_cover, 32), name
        read = pos.client_verify_read(root, len(data), PRE, ENC, a, b, rows_msg, COLS, opening, seed=7)
        assert read == data[a:b], name
        got, dots, ok = pos.segment_leaves(opening.segments, rows, plan.chunk_lo, plan.chunk_hi, opening.covers)
        assert dots is None and ok.all()
        assert [got[k].tobytes() for k in range(len(COLS))] == leaves, name
        if name in ("first", "last"):
            # eight covers under the 256-chunk subtree; the 257th chunk is a cover of its own, or the one read
            n_cover = {("first", 256): 8, ("last", 256): 8, ("first", 257): 9, ("last", 257): 1}[name, n]
            assert plan.chunk_hi - plan.chunk_lo == 1 and plan.n_cover == n_cover, name
            assert [int(v) for v in opening.segments[1]] == column[plan.seg_row_lo:plan.seg_row_hi]
            want = [R._words(R.subtree_cv(ref_cvs, lo, hi)) for lo, hi in want_plan["cover_nodes"]]
            assert [opening.covers[1, j].tobytes() for j in range(plan.n_cover)] == want, name
            assert R.leaf_from_opening(rows, plan.chunk_lo, plan.chunk_hi, column[plan.seg_row_lo:plan.seg_row_hi],
                                       want) == leaves[1], name
            for j in (0, plan.n_cover - 1):
                forged = copy.deepcopy(opening)
                forged.covers[2, j, 31] ^= 0x80
                with pytest.raises(pos.VerifierError) as e:
                    pos.client_verify_read(root, len(data), PRE, ENC, a, b, rows_msg, COLS, forged, seed=7)
                assert e.value.kind == "ColumnEval", (name, j)
