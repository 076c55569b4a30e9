"""CPU: the host-only parts of the PoS column chunk-CV cache (pos_files.ColumnChunkCache over
lcpc_pos_chunk_cache_*): the rehash rule lcpc_pos_update_chunk_range against a brute-force
description of the BLAKE3 chunks, the `.porcv` sidecar header, and the new C-ABI symbols.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")

NEW_SYMBOLS = [
    "lcpc_pos_update_chunk_range", "lcpc_pos_chunk_cache_from_porenc", "lcpc_pos_chunk_cache_from_cvs",
    "lcpc_pos_chunk_cache_free", "lcpc_pos_chunk_cache_enc", "lcpc_pos_chunk_cache_rows",
    "lcpc_pos_chunk_cache_n_chunks", "lcpc_pos_chunk_cache_copy_cvs", "lcpc_pos_chunk_cache_update", "lcpc_pos_chunk_cache_update_fd",
    "lcpc_pos_chunk_cache_tree", "lcpc_pos_writer_n_chunks", "lcpc_pos_writer_copy_cvs", "lcpc_leaves_fold_cvs",
]


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", PKG], check=True)
    N.load()
    return N


@pytest.fixture(scope="module")
def PF(native):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


# ---------------------------------------------------------------- the rehash rule
def _chunks(rows):
    """Every 1-KiB chunk of the column message 32 zero bytes || rows 8-byte elements, as what its
    chaining value depends on besides the bytes: (first byte, end byte, length, counter, only chunk)."""
    total = 32 + 8 * rows
    n = max(1, -(-total // 1024))
    return [(1024 * c, min(total, 1024 * (c + 1)), min(total, 1024 * (c + 1)) - 1024 * c, c, n == 1)
            for c in range(n)]


def _chunk_rows(desc):
    """rows whose 8 bytes [32 + 8 r, 40 + 8 r) lie in the chunk (elements never straddle: 8 | 1024)"""
    b0, b1 = desc[0], desc[1]
    return range(max(0, (b0 - 32) // 8), max(0, (b1 - 32) // 8))


def _dirty(old_rows, new_rows, row_lo, row_hi):
    old, new = _chunks(old_rows), _chunks(new_rows)
    out = set()
    for c, d in enumerate(new):
        rows = _chunk_rows(d)
        touched = row_lo < row_hi and rows.start < row_hi and row_lo < rows.stop
        if c >= len(old) or old[c] != d or touched:
            out.add(c)
    return out


GRID = [0, 1, 2, 60, 123, 124, 125, 126, 200, 251, 252, 253, 254, 300, 379, 380, 381, 400]


def _row_ranges(old_rows, new_rows):
    cand = [(0, 0), (0, 1), (0, new_rows), (new_rows - 1, new_rows), (old_rows, new_rows), (old_rows - 1, new_rows),
            (123, 124), (123, 125), (124, 125), (251, 252), (251, 253), (252, 253), (60, 61), (200, 300),
            (100, 390), (379, 381), (new_rows, new_rows)]
    return sorted({(a, b) for a, b in cand if 0 <= a <= b <= new_rows})


def test_update_chunk_range_against_brute_force(PF):
    rng = PF.ColumnChunkCache.update_chunk_range
    cases = 0
    for old_rows in GRID:
        for new_rows in GRID:
            if new_rows < old_rows:
                continue
            old_last = len(_chunks(old_rows)) - 1
            for row_lo, row_hi in _row_ranges(old_rows, new_rows):
                lo, hi = rng(old_rows, new_rows, row_lo, row_hi)
                dirty = _dirty(old_rows, new_rows, row_lo, row_hi)
                what = (old_rows, new_rows, row_lo, row_hi, lo, hi, sorted(dirty))
                cases += 1
                if not dirty:
                    assert new_rows == old_rows and lo == hi, what
                    continue
                # every dirty chunk is rehashed ...
                assert lo <= min(dirty) and max(dirty) < hi <= len(_chunks(new_rows)), what
                # ... and nothing past the last dirty one; before the first, at most the old last
                # chunk on growth (the stated rule takes it whether or not its length changed)
                assert hi == max(dirty) + 1, what
                floor = min(min(dirty), old_last) if new_rows > old_rows else min(dirty)
                assert lo >= floor, what
    assert cases > 1500


def test_update_chunk_range_known_cases(PF):
    rng = PF.ColumnChunkCache.update_chunk_range
    assert rng(300, 300, 0, 1) == (0, 1)
    assert rng(300, 300, 123, 125) == (0, 2)       # rows 123 | 124 straddle chunks 0 and 1
    assert rng(300, 300, 251, 253) == (1, 3)
    assert rng(300, 300, 299, 300) == (2, 3)
    assert rng(0, 1, 0, 1) == (0, 1)               # from the empty message
    assert rng(124, 125, 124, 125) == (0, 2)       # chunk 0 was the only chunk: it loses ROOT
    assert rng(252, 253, 252, 253) == (1, 3)       # the old last chunk, by the rule
    assert rng(100, 400, 100, 400) == (0, 4)
    assert rng(300, 400, 10, 11) == (0, 4)         # an edit before the old last chunk, with growth
    assert rng(300, 300, 5, 5) == (0, 0)           # nothing to do


@pytest.mark.parametrize("args", [(300, 299, 0, 1), (300, 300, 0, 301), (300, 300, 5, 4), (1, 0, 0, 0)])
def test_update_chunk_range_rejects(PF, args):
    from lcpc_proof_of_storage_amd import lcpc2d
    with pytest.raises((ValueError, lcpc2d.LcpcError)):
        PF.ColumnChunkCache.update_chunk_range(*args)


def test_leaf_n_chunks_matches_library(PF, native):
    for rows in list(range(0, 520)) + [9363, 1 << 20]:
        assert PF.leaf_n_chunks(rows) == native.load().lcpc_leaf_n_chunks(0, rows), rows


# ---------------------------------------------------------------- sidecar header
def test_sidecar_header_round_trip(PF):
    root = bytes(range(32))
    h = PF.encode_chunk_cv_header(32768, 9363, 74, root)
    assert len(h) == PF.CHUNK_CV_HEADER_BYTES == 64 and h[:8] == PF.CHUNK_CV_MAGIC
    assert PF.parse_chunk_cv_header(h) == (32768, 9363, 74, root)
    assert PF.parse_chunk_cv_header(h + b"body") == (32768, 9363, 74, root)
    full = 64 + 74 * 32768 * 32
    assert PF.check_chunk_cv_sidecar(h, full, 32768, 9363, root) == 74
    assert PF.check_chunk_cv_sidecar(h, full + 5, 32768, 9363, root) == 74
    with pytest.raises(ValueError):
        PF.encode_chunk_cv_header(4, 1, 1, b"short")


def test_sidecar_header_rejections(PF):
    root = bytes(range(32))
    h = PF.encode_chunk_cv_header(8, 300, 3, root)
    full = 64 + 3 * 8 * 32
    PF.check_chunk_cv_sidecar(h, full, 8, 300, root)
    with pytest.raises(ValueError, match="magic"):
        PF.check_chunk_cv_sidecar(b"PORCV\0\0\2" + h[8:], full, 8, 300, root)
    with pytest.raises(ValueError, match="magic"):
        PF.parse_chunk_cv_header(bytes(64))
    with pytest.raises(ValueError, match="shorter"):
        PF.parse_chunk_cv_header(h[:63])
    with pytest.raises(ValueError, match="dimensions"):
        PF.check_chunk_cv_sidecar(h, full, 16, 300, root)          # another enc
    with pytest.raises(ValueError, match="dimensions"):
        PF.check_chunk_cv_sidecar(h, full, 8, 301, root)           # another row count
    with pytest.raises(ValueError, match="dimensions"):             # a chunk count that is not the rows'
        PF.check_chunk_cv_sidecar(PF.encode_chunk_cv_header(8, 300, 2, root), full, 8, 300, root)
    with pytest.raises(ValueError, match="short"):
        PF.check_chunk_cv_sidecar(h, full - 1, 8, 300, root)
    with pytest.raises(ValueError, match="root"):
        PF.check_chunk_cv_sidecar(h, full, 8, 300, bytes(32))


def test_sidecar_file_whole_and_partial_writes(PF, tmp_path):
    import numpy as np
    rng = np.random.default_rng(5)
    enc, rows = 4, 300
    cvs = rng.integers(0, 256, (3, enc, 32), dtype=np.uint8)
    p = str(tmp_path / "x.porcv")
    with pytest.raises(FileNotFoundError):
        PF.write_chunk_cv_sidecar(p, enc, rows, bytes(32), cvs[1:2], 1)
    PF.write_chunk_cv_sidecar(p, enc, rows, b"\1" * 32, cvs)
    data = open(p, "rb").read()
    assert PF.check_chunk_cv_sidecar(data[:64], len(data), enc, rows, b"\1" * 32) == 3
    assert data[64:] == cvs.tobytes()
    # chunk row 0 alone is rewritten (an edit of row 0), then the file grows by two chunk rows
    new0 = rng.integers(0, 256, (1, enc, 32), dtype=np.uint8)
    PF.write_chunk_cv_sidecar(p, enc, rows, b"\2" * 32, new0, 0)
    data = open(p, "rb").read()
    assert data[64:] == new0.tobytes() + cvs[1:].tobytes()
    assert PF.parse_chunk_cv_header(data)[3] == b"\2" * 32
    tail = rng.integers(0, 256, (3, enc, 32), dtype=np.uint8)
    PF.write_chunk_cv_sidecar(p, enc, 600, b"\3" * 32, tail, 2)
    data = open(p, "rb").read()
    assert PF.check_chunk_cv_sidecar(data[:64], len(data), enc, 600, b"\3" * 32) == 5
    assert data[64:] == new0.tobytes() + cvs[1:2].tobytes() + tail.tobytes()
    with pytest.raises(ValueError):
        PF.write_chunk_cv_sidecar(p, enc, 600, b"\3" * 32, tail, 3)


# ---------------------------------------------------------------- C ABI
def test_new_symbols_declared_exported_bound(native):
    import ctypes as C
    declared = set(native.header_symbols())
    raw = C.CDLL(native.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in native.SIGNATURES, s
    assert native.load().lcpc_abi_version() >= 2
