"""CPU: the checkable read's reference (read_ref.py) against pyref's BLAKE3, the host-only plan
lcpc_pos_read_plan against the reference, and the new C-ABI symbols (which, the plan apart, need a
device)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import read_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")
INVALID_ARG, NO_DEVICE = 30, 33

NEW_SYMBOLS = ["lcpc_pos_read_plan", "lcpc_pos_segment_covers_from_cache", "lcpc_pos_segment_covers_from_columns",
               "lcpc_pos_segment_leaves"]

# one chunk; two chunks with the boundary row on either side; three, left-balanced; a ragged last
# chunk; nine and ten chunks (a tree of depth 4 whose right spine is ragged)
ROW_COUNTS = [1, 124, 125, 253, 381, 700, 1100, 1149]


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", PKG], check=True)
    N.load()
    return N


@pytest.fixture(scope="module")
def pos(native):
    from lcpc_proof_of_storage_amd import pos as P
    return P


def _column(rows, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, R.P, rows, dtype=np.uint64)]


@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_every_chunk_range_rebuilds_the_leaf(rows):
    col = _column(rows, rows)
    want = R.leaf(col)
    n = R.n_chunks(rows)
    assert R.subtree_cv(R.column_chunk_cvs(col), 0, n, True) == [int.from_bytes(want[4 * i:4 * i + 4], "little")
                                                               for i in range(8)]
    most = 0
    for lo in range(n):
        for hi in range(lo + 1, n + 1):
            cov = R.covers(col, lo, hi)
            most = max(most, len(cov))
            assert len(cov) <= max(0, 2 * (n - 1).bit_length())
            seg_lo = R.chunk_first_row(lo)
            seg_hi = rows if hi == n else R.chunk_first_row(hi)
            assert R.leaf_from_opening(rows, lo, hi, col[seg_lo:seg_hi], cov) == want, (rows, lo, hi)
    assert (most == 0) == (n == 1)


def test_cover_nodes_partition_the_rest():
    for n in (1, 2, 3, 5, 9, 10, 74, 75, 1000):
        for lo, hi in {(0, 1), (n - 1, n), (n // 2, n // 2 + 1), (0, n), (n // 3, max(n // 3 + 1, 2 * n // 3))}:
            nodes = R.cover_nodes(n, lo, hi)
            covered = sorted(c for a, b in nodes for c in range(a, b))
            assert covered == [c for c in range(n) if not lo <= c < hi], (n, lo, hi)
            assert nodes == sorted(nodes) and len(nodes) <= 2 * max(1, (n - 1).bit_length())
            if (lo, hi) == (0, n) or n == 1:
                assert nodes == []


def _plan_grid():
    for pre in (1, 8, 64, 16384):
        rb = 7 * pre
        for file_len in (1, rb - 1, rb, rb + 1, 124 * rb, 124 * rb + 1, 125 * rb + 3, 700 * rb - 5, 1149 * rb):
            if file_len > (1 << 31):
                continue
            rows = -(-(-(-file_len // 7)) // pre)
            ranges = {(0, 1), (0, file_len), (file_len - 1, file_len),          # one byte; all; the last byte
                      (0, min(rb, file_len)),                                   # ends on a row boundary
                      ((rows - 1) * rb, file_len),                              # the (ragged) last row
                      (min(rb - 1, file_len - 1), min(rb + 1, file_len)),       # across rows 0 | 1
                      (min(123 * rb, file_len - 1), min(125 * rb, file_len)),   # across chunks 0 | 1
                      (file_len // 2, file_len // 2 + 1), (file_len // 3, max(file_len // 3 + 1, 2 * file_len // 3))}
            for a, b in sorted(ranges):
                if 0 <= a < b <= file_len:
                    yield file_len, a, b, pre


def test_read_plan_against_the_reference(pos):
    cases = 0
    for file_len, a, b, pre in _plan_grid():
        want = R.read_plan(file_len, a, b, pre)
        got = pos.read_plan(file_len, a, b, pre)
        for k in ("row_lo", "row_hi", "chunk_lo", "chunk_hi", "seg_row_lo", "seg_row_hi"):
            assert getattr(got, k) == want[k], (file_len, a, b, pre, k)
        assert got.cover_nodes == want["cover_nodes"] and got.n_cover == len(want["cover_nodes"])
        # the rows read lie inside the segment, the segment inside the file
        assert want["seg_row_lo"] <= want["row_lo"] < want["row_hi"] <= want["seg_row_hi"] <= want["rows"]
        cases += 1
    assert cases > 150
    one_row = pos.read_plan(5, 0, 5, 8)
    assert (one_row.row_lo, one_row.row_hi, one_row.chunk_lo, one_row.chunk_hi, one_row.seg_row_lo,
            one_row.seg_row_hi, one_row.cover_nodes) == (0, 1, 0, 1, 0, 1, [])


@pytest.mark.parametrize("args", [(100, 5, 5, 8), (100, 6, 5, 8), (100, 0, 101, 8), (100, 0, 10, 0)])
def test_read_plan_rejects(native, args):
    r = [C.c_size_t() for _ in range(7)]
    assert native.load().lcpc_pos_read_plan(*args, *[C.byref(v) for v in r], None, 0) == INVALID_ARG


def test_read_plan_cover_capacity(native):
    lib = native.load()
    n = C.c_size_t()
    file_len = 7 * 8 * 1149
    assert lib.lcpc_pos_read_plan(file_len, 7 * 8 * 600, 7 * 8 * 600 + 1, 8, None, None, None, None, None, None,
                                  C.byref(n), None, 0) == 0
    assert n.value == len(R.cover_nodes(10, 4, 5)) >= 2
    nodes = (C.c_size_t * (2 * n.value))()
    assert lib.lcpc_pos_read_plan(file_len, 7 * 8 * 600, 7 * 8 * 600 + 1, 8, None, None, None, None, None, None,
                                  None, nodes, n.value - 1) == INVALID_ARG
    assert lib.lcpc_pos_read_plan(file_len, 7 * 8 * 600, 7 * 8 * 600 + 1, 8, None, None, None, None, None, None,
                                  None, nodes, n.value) == 0
    assert [(nodes[2 * j], nodes[2 * j + 1]) for j in range(n.value)] == R.cover_nodes(10, 4, 5)


def test_new_symbols_declared_exported_bound(native):
    declared = set(native.header_symbols())
    raw = C.CDLL(native.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in native.SIGNATURES, s
    assert native.load().lcpc_abi_version() == 3


def test_compute_entries_need_a_device(native, pos):
    """Without a GPU the compute entries report LCPC_ERR_NO_DEVICE (the plan alone is host-only); with
    one, the same valid calls succeed.  Bad arguments are refused either way."""
    lib = native.load()
    NO_DEVICE = 33 if lib.lcpc_device_count() <= 0 else 0  # noqa: N806
    rows = 300
    cols = np.zeros((2, rows), np.uint64)
    out = np.zeros((2, 2, 32), np.uint8)
    u8 = lambda a: a.ctypes.data_as(native.u8p)  # noqa: E731
    u64 = lambda a: a.ctypes.data_as(native.u64p)  # noqa: E731
    assert lib.lcpc_pos_segment_covers_from_columns(u64(cols), rows, 2, 1, 2, u8(out)) == NO_DEVICE
    seg = np.zeros((2, 128), np.uint64)
    leaves, ok = np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    assert lib.lcpc_pos_segment_leaves(u64(seg), 2, rows, 1, 2, u8(out), 2, None, u8(leaves), None, u8(ok)) == NO_DEVICE
    if NO_DEVICE:
        with pytest.raises(pos.DeviceError) as e:
            pos.segment_leaves(seg, rows, 1, 2, out)
        assert e.value.code == NO_DEVICE
    # argument checks come first
    assert lib.lcpc_pos_segment_leaves(u64(seg), 2, rows, 1, 2, u8(out), 1, None, u8(leaves), None, u8(ok)) == INVALID_ARG
    assert lib.lcpc_pos_segment_leaves(u64(seg), 2, rows, 2, 2, u8(out), 2, None, u8(leaves), None, u8(ok)) == INVALID_ARG
    assert lib.lcpc_pos_segment_leaves(u64(seg), 2, rows, 1, 4, u8(out), 2, None, u8(leaves), None, u8(ok)) == INVALID_ARG
    assert lib.lcpc_pos_segment_covers_from_cache(None, None, 0, 0, 1, None) == INVALID_ARG
