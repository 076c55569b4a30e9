"""Pure-Python reference of the checkable read (include/lcpc_mi.h, "PoS checkable reads"): the plan
of a byte range, the cover walk over BLAKE3's left-balanced chunk tree, and a column's leaf rebuilt
from a segment and its covers -- all over pyref.compress / pyref._chunk_cv."""
import pyref

P = pyref.FIELD_DECL[0][0]          # WriteableFt63's modulus
R_INV = pow(1 << 64, -1, P)         # Montgomery limbs x hold the value x / 2^64
PARENT, ROOT = 4, 8


def from_mont(x: int) -> int:
    return int(x) * R_INV % P


def n_chunks(rows: int) -> int:
    return max(1, -(-(32 + 8 * rows) // 1024))


def chunk_first_row(chunk: int) -> int:
    return 0 if chunk == 0 else 128 * chunk - 4


def chunk_of_row(row: int) -> int:
    return (32 + 8 * row) // 1024


def cover_nodes(n: int, chunk_lo: int, chunk_hi: int):
    """The disjoint nodes of the walk from [0, n), in order."""
    out = []

    def walk(lo, hi):
        if hi <= chunk_lo or lo >= chunk_hi:
            out.append((lo, hi))
        elif not (chunk_lo <= lo and hi <= chunk_hi):
            half = 1
            while 2 * half < hi - lo:
                half *= 2
            walk(lo, lo + half)
            walk(lo + half, hi)

    walk(0, n)
    return out


def read_plan(file_len: int, byte_start: int, byte_end: int, pre: int) -> dict:
    assert 0 <= byte_start < byte_end <= file_len and pre > 0
    rb = 7 * pre
    rows = -(-(-(-file_len // 7)) // pre)
    n = n_chunks(rows)
    row_lo, row_hi = byte_start // rb, -(-byte_end // rb)
    chunk_lo, chunk_hi = chunk_of_row(row_lo), chunk_of_row(row_hi - 1) + 1
    return dict(rows=rows, n_chunks=n, row_lo=row_lo, row_hi=row_hi, chunk_lo=chunk_lo, chunk_hi=chunk_hi,
                seg_row_lo=chunk_first_row(chunk_lo),
                seg_row_hi=rows if chunk_hi == n else chunk_first_row(chunk_hi),
                cover_nodes=cover_nodes(n, chunk_lo, chunk_hi))


def _message(column) -> bytes:
    return bytes(32) + b"".join(int(v).to_bytes(8, "little") for v in column)


def _words(cv) -> bytes:
    return b"".join(x.to_bytes(4, "little") for x in cv)


def _parent(left, right, root: bool):
    return pyref.compress(pyref.IV, _words(left) + _words(right), 0, 64, PARENT | (ROOT if root else 0))


def subtree_cv(chunk_cvs, lo: int, hi: int, root: bool = False):
    """The node over chunks [lo, hi) from their chaining values (chunk_cvs[c] for lo <= c < hi)."""
    if hi - lo == 1:
        return chunk_cvs[lo]
    half = 1
    while 2 * half < hi - lo:
        half *= 2
    return _parent(subtree_cv(chunk_cvs, lo, lo + half), subtree_cv(chunk_cvs, lo + half, hi), root)


def column_chunk_cvs(column):
    """Every chunk's chaining value of the column's leaf message (canonical integer elements)."""
    msg = _message(column)
    n = n_chunks(len(column))
    return [pyref._chunk_cv(msg[1024 * c:1024 * (c + 1)], c, n == 1) for c in range(n)]


def covers(column, chunk_lo: int, chunk_hi: int):
    """The server's cover values of a whole column opened on [chunk_lo, chunk_hi): 32 bytes each."""
    cvs = column_chunk_cvs(column)
    return [_words(subtree_cv(cvs, lo, hi)) for lo, hi in cover_nodes(len(cvs), chunk_lo, chunk_hi)]


def leaf_from_opening(rows: int, chunk_lo: int, chunk_hi: int, segment, cover_values) -> bytes:
    """The client's leaf: segment = the elements of rows [first row of chunk_lo, first row of
    chunk_hi or rows), hashed with their true chunk counters, folded with the covers along the walk."""
    n = n_chunks(rows)
    seg_lo = chunk_first_row(chunk_lo)
    # the chunk's bytes: the 32-byte prefix belongs to chunk 0 only
    body = b"".join(int(v).to_bytes(8, "little") for v in segment)
    stream = (bytes(32) if chunk_lo == 0 else b"") + body
    base = 1024 * chunk_lo
    cvs = {c: pyref._chunk_cv(stream[1024 * c - base:1024 * (c + 1) - base], c, n == 1)
           for c in range(chunk_lo, chunk_hi)}
    assert seg_lo * 8 + 32 == base or chunk_lo == 0
    it = iter(cover_values)

    def walk(lo, hi, root):
        if hi <= chunk_lo or lo >= chunk_hi:
            cover = next(it)
            return [int.from_bytes(cover[4 * i:4 * i + 4], "little") for i in range(8)]
        if chunk_lo <= lo and hi <= chunk_hi:
            return subtree_cv(cvs, lo, hi, root)
        half = 1
        while 2 * half < hi - lo:
            half *= 2
        left = walk(lo, lo + half, False)
        return _parent(left, walk(lo + half, hi, False), root)

    leaf = walk(0, n, True)
    assert next(it, None) is None, "more covers than the walk takes"
    return _words(leaf)


def leaf(column) -> bytes:
    """BLAKE3(32 zero bytes || column) by pyref's own hasher."""
    return pyref.blake3(_message(column))
