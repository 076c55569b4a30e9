"""Mutation builder for the verifier sweeps (checker only: NumPy, Python integers, oracle_ffi and
batch_ref; nothing here runs the product).

A verifier is sound only if every opened column, row, word, path level, root byte and claimed value
reaches its verdict.  The per-column checks of verify (lcpc-2d/src/lib.rs:953-974) come in a fixed
order -- the degree tests <T_i, col> (ColumnDegree), the evaluation <u, col> (ColumnEval), the Merkle
path of the column's leaf (ColumnPath) -- so a changed column word normally dies at the first of them
and never shows that the later ones bind the column.  This module separates them.  For a proof with
degree-test tensors T_i and outer tensor(s) u_j, a vector delta is added to one opened column:

  RAW           delta = s e_r                                  -> ColumnDegree (ColumnEval when there
                                                                  are no degree tests)
  DEGREE_BLIND  <T_i, delta> = 0 for all i, <u_j, delta> != 0  -> ColumnEval (naming evaluation j)
  ALL_BLIND     <T_i, delta> = 0 and <u_j, delta> = 0          -> ColumnPath: only the leaf hash sees it

delta is supported on the target row and as many helper rows as there are vectors to be blind to; the
helper values solve an exact linear system mod p on Python integers (blind).  The mutated column is
to_mont((from_mont(col) + delta) mod p): every word stays a reduced field element.

The kernels compare sums with the encoded vectors' entries as stored (Montgomery) words.  RAW_TOP is
RAW with the scale that moves the column's first check by one unit of its top stored word only, and
shift_stored changes a claimed value in one stored word: a comparison that skips a word lets them by.

T_i and the opened column indices depend only on the transcript's seed, p_random and p_eval, never on
the columns (replay), so one replay serves every column mutation of a proof.

The place lists name where kernels go wrong: the opened columns around a 64-lane boundary of the
check kernels, the rows at the ends of every 1-KiB leaf chunk and of the first 64-byte block, every
32-bit word of an element, every path level, every root byte.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Callable, Dict, Iterator, List, Optional, Sequence

import numpy as np

import batch_ref as B
import oracle_ffi as O

RAW, DEGREE_BLIND, ALL_BLIND = "RAW", "DEGREE_BLIND", "ALL_BLIND"
RAW_TOP = "RAW_TOP"   # RAW scaled so that the first check's sum moves in its top stored word only
PATH, ROOT, EXCHANGE, P_EVAL, P_RANDOM = "PATH", "ROOT", "EXCHANGE", "P_EVAL", "P_RANDOM"
COLUMN_CLASSES = (RAW, DEGREE_BLIND, ALL_BLIND)

OK, COLUMN_PATH, COLUMN_EVAL, COLUMN_DEGREE = B.OK, B.COLUMN_PATH, B.COLUMN_EVAL, B.COLUMN_DEGREE
KIND = {OK: "OK", B.NUM_COL_OPENS: "NumColOpens", COLUMN_PATH: "ColumnPath", COLUMN_EVAL: "ColumnEval",
        COLUMN_DEGREE: "ColumnDegree", B.OUTER_TENSOR: "OuterTensor", B.INNER_TENSOR: "InnerTensor",
        16: "EncodingDims", 17: "Encode"}

FIELD_IDS = (0, 1, 2, 3, 4)  # Ft63, Ft127, Ft191, Ft255, Ft253_192
CHUNK_WORDS, PREFIX_WORDS, BLOCK_WORDS = 256, 8, 16  # a BLAKE3 chunk, the leaf's 32 zero bytes, a block


# ---------------------------------------------------------------- shapes
def field_words(fid: int) -> int:
    """32-bit words of an element's repr in the leaf message"""
    return 2 * O.limbs(fid)


def n_chunks(fid: int, n_rows: int) -> int:
    """lcpc_leaf_n_chunks: 1-KiB chunks of the leaf message (32 zero bytes, then every element)"""
    return (PREFIX_WORDS + n_rows * field_words(fid) + CHUNK_WORDS - 1) // CHUNK_WORDS


def rows_for_chunks(fid: int, chunks: int) -> int:
    """the smallest row count whose leaf has `chunks` chunks: its last chunk holds exactly one element
    (for Ft191 the tail of the element that straddles the chunk edge); chunks = 1 gives the largest
    one-chunk column instead, a chunk filled to its last whole element"""
    fw = field_words(fid)
    if chunks == 1:
        return (CHUNK_WORDS - PREFIX_WORDS) // fw
    return (CHUNK_WORDS * (chunks - 1) - PREFIX_WORDS) // fw + 1


@dataclass(frozen=True)
class Shape:
    name: str
    n_per_row: int
    n_cols: int
    n_open: int
    n_rows: int
    thin_rows: bool = False  # the 9- and 17-chunk shapes keep the chunk-boundary rows only


N_PER_ROW, N_COLS, N_OPEN = 8, 128, 70   # path_len 7, two lanes past a 64-lane group
ONE_ROW = Shape("row1", 8, 16, 6, 1)
NDTS = (0, 1, 3)
CHUNK_CLASSES = {fid: ((1, 2, 3, 9, 17) if fid in (0, 2) else (1, 2, 3)) for fid in FIELD_IDS}


def single_shapes(fid: int, chunks: int) -> List[Shape]:
    """the row counts of one (field, chunk count) case.  Ft63 columns are 16-byte aligned only for an
    even row count (the column-major leaf kernel, with its two-chunk form); an odd one falls into the
    strided kernel, so Ft63 takes both up to 9 chunks (at 17 the merge in groups is what is new, and
    it does not see the layout)."""
    n = rows_for_chunks(fid, chunks)
    rows = [n]
    if fid == 0 and chunks <= 9:
        rows.append(n - 1 if chunks == 1 else n + 1)
    return [Shape(f"c{chunks}r{r}", N_PER_ROW, N_COLS, N_OPEN, r, thin_rows=chunks >= 9) for r in rows]


# the batch sweep (Ft127, Ft191): a three-chunk column
BATCH_FIELDS, BATCH_MS, BATCH_NDTS = (1, 2), (1, 3), (0, 2)


def batch_shape(fid: int) -> Shape:
    return single_shapes(fid, 3)[0]


# ---------------------------------------------------------------- place lists
def opened_places(n_open: int, flags_per_col: int) -> List[int]:
    """opened columns at the ends of a 64-lane group of the one-column-per-lane kernels, and the
    columns one of whose (column, tensor) flags is number 63 or 64 (k_column_checks runs 64-thread
    blocks over the pairs, flags_per_col of them per column)"""
    ks = {0, 1, 62, 63, 64, 65, n_open - 1}
    for k in range(n_open):
        if any(k * flags_per_col + t in (63, 64) for t in range(flags_per_col)):
            ks.add(k)
    return sorted(k for k in ks if 0 <= k < n_open)


def chunk_rows(fid: int, n_rows: int) -> List[tuple]:
    """(first, last) row with a word in each chunk; an element that straddles a chunk edge (Ft191)
    counts for both chunks"""
    fw, out = field_words(fid), []
    for c in range(n_chunks(fid, n_rows)):
        lo = max(CHUNK_WORDS * c - PREFIX_WORDS, 0) // fw
        hi = min((CHUNK_WORDS * (c + 1) - 1 - PREFIX_WORDS) // fw, n_rows - 1)
        out.append((lo, hi))
    return out


def row_places(fid: int, n_rows: int, thin: bool = False) -> List[int]:
    fw = field_words(fid)
    rows = {r for pair in chunk_rows(fid, n_rows) for r in pair}
    if not thin:
        rows |= {0, 1, n_rows - 1}
        # the rows holding the last word of the first 64-byte block and the first word of the second
        rows |= {(BLOCK_WORDS - 1 - PREFIX_WORDS) // fw, (BLOCK_WORDS - PREFIX_WORDS) // fw}
    return sorted(r for r in rows if 0 <= r < n_rows)


def word_rows(fid: int, n_rows: int) -> List[int]:
    """one row per chunk: the last with a word in it"""
    return sorted({hi for _, hi in chunk_rows(fid, n_rows)})


def word_scales(fid: int) -> List[int]:
    return [1 << (32 * w) for w in range(field_words(fid))]


PATH_BYTES = (0, 15, 31)


# ---------------------------------------------------------------- exact arithmetic mod p
def canon(fid: int, elems) -> List[int]:
    return O.from_mont(fid, np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1))


def dot(v: Sequence[int], delta: Sequence[int], p: int) -> int:
    return sum(a * d for a, d in zip(v, delta) if d) % p


def _solve(a: List[List[int]], b: List[int], p: int) -> Optional[List[int]]:
    """x with a x = b mod p (a square), or None when a is singular"""
    n = len(a)
    m = [list(row) + [rhs] for row, rhs in zip(a, b)]
    for c in range(n):
        piv = next((r for r in range(c, n) if m[r][c] % p), None)
        if piv is None:
            return None
        m[c], m[piv] = m[piv], m[c]
        inv = pow(m[c][c], -1, p)
        m[c] = [v * inv % p for v in m[c]]
        for r in range(n):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(v - f * w) % p for v, w in zip(m[r], m[c])]
    return [m[r][n] for r in range(n)]


def blind(vectors: Sequence[Sequence[int]], target_row: int, scale: int, n_rows: int, p: int) -> List[int]:
    """delta (canonical integers, n_rows of them) with delta[target_row] = scale, supported on the
    target and len(vectors) helper rows, and <v, delta> = 0 mod p for every v.  The helper rows are the
    rows after the target (cyclically); if they make the system singular the window moves on, and only
    when every window is singular is that an error: a case is never skipped."""
    h = len(vectors)
    if n_rows < h + 1:
        raise ValueError(f"{h} vectors need {h + 1} rows, the column has {n_rows}")
    scale %= p
    assert scale, "a zero scale changes nothing"
    others = [(target_row + 1 + i) % n_rows for i in range(n_rows - 1)]
    for start in range(len(others) - h + 1):
        rows = others[start:start + h]
        x = _solve([[v[r] % p for r in rows] for v in vectors], [(-scale * v[target_row]) % p for v in vectors], p)
        if x is None:
            continue
        delta = [0] * n_rows
        delta[target_row] = scale
        for r, v in zip(rows, x):
            delta[r] = v
        assert all(dot(v, delta, p) == 0 for v in vectors)
        return delta
    raise ArithmeticError("every choice of helper rows is singular")


def add_delta(fid: int, col: np.ndarray, delta: Sequence[int], p: int) -> np.ndarray:
    """to_mont((from_mont(col) + delta) mod p), same shape as col"""
    nl = O.limbs(fid)
    out = np.array(col, dtype=np.uint64, copy=True)
    view = out.reshape(-1, nl)
    rows = [r for r, d in enumerate(delta) if d]
    cur = O.from_mont(fid, np.ascontiguousarray(view[rows]).reshape(-1))
    view[rows] = O.to_mont(fid, [(c + delta[r]) % p for c, r in zip(cur, rows)]).reshape(-1, nl)
    return out


def shift_value(fid: int, elem: np.ndarray, word: int, p: int) -> np.ndarray:
    """a claimed value changed by 2^(32 word), down instead of up where up would reach p"""
    v = canon(fid, elem)[0]
    s = 1 << (32 * word)
    assert s < p
    w = v + s if v + s < p else v - s
    assert 0 <= w < p and w != v
    return O.to_mont(fid, [w]).reshape(np.asarray(elem).shape)


def stored_int(fid: int, elem) -> int:
    """the integer an element's stored (Montgomery) limbs spell"""
    return O.ints_from_limbs(np.ascontiguousarray(elem, dtype=np.uint64).reshape(-1), O.limbs(fid))[0]


def shift_stored(fid: int, elem: np.ndarray, word: int, p: int) -> np.ndarray:
    """an element whose STORED words differ from elem's in 32-bit word `word` alone (and upwards, by
    carry): the stored integer plus 2^(32 word), or minus where plus would reach p.  The kernels
    compare stored words (fe_eq), and a canonical change of 2^(32 word) spreads over all of them."""
    v = stored_int(fid, elem)
    s = 1 << (32 * word)
    assert s < p
    w = v + s if v + s < p else v - s
    assert 0 <= w < p
    return O.limbs_from_ints([w], O.limbs(fid)).reshape(np.asarray(elem).shape)


def other_element(fid: int, elem: np.ndarray, p: int) -> np.ndarray:
    """another reduced element: the value plus one"""
    return O.to_mont(fid, [(canon(fid, elem)[0] + 1) % p]).reshape(np.asarray(elem).shape)


def flip(data: bytes, byte: int, bit: int) -> bytes:
    out = bytearray(data)
    out[byte] ^= 1 << (bit % 8)
    return bytes(out)


# ---------------------------------------------------------------- proofs as plain words
def as_batch(pf) -> "B.BatchProof":
    """an oracle Proof as a batch_ref.BatchProof with one evaluation (copies)"""
    if isinstance(pf, B.BatchProof):
        return pf
    nco, pl = pf.n_col_opens, pf.path_len
    cols = pf.cols.copy().reshape(nco, -1)
    paths = pf.paths.tobytes()
    pr = pf.p_random.copy().reshape(pf.n_degree_tests, -1) if pf.n_degree_tests else []
    return B.BatchProof(pf.fid, pf.n_cols, [pf.p_eval.copy()], [r for r in pr], [int(c) for c in pf.col_idx],
                        [cols[k] for k in range(nco)], [paths[32 * pl * k:32 * pl * (k + 1)] for k in range(nco)])


def as_oracle(bp: "B.BatchProof", n_open: int) -> "O.Proof":
    """a one-evaluation BatchProof as the C oracle's proof"""
    assert len(bp.p_evals) == 1 and len(bp.cols) == n_open
    nl = O.limbs(bp.fid)
    flat = [np.asarray(c, dtype=np.uint64).reshape(-1) for c in bp.cols]
    pr = np.concatenate([np.asarray(r, dtype=np.uint64).reshape(-1) for r in bp.p_random]) if bp.p_random \
        else np.zeros(0, np.uint64)
    pe = np.asarray(bp.p_evals[0], dtype=np.uint64).reshape(-1)
    return O.Proof.from_parts(bp.fid, bp.n_cols, pe.size // nl, flat[0].size // nl, pe, pr, np.concatenate(flat),
                              np.frombuffer(b"".join(bp.paths), np.uint8), len(bp.p_random), n_open,
                              len(bp.paths[0]) // 32)


def replay(proof, root: bytes, n_open: int, make_tr: Optional[Callable] = None):
    """(degree-test tensors, opened column indices) the verifier draws for this proof: they depend on
    the transcript's seed (make_tr, by default the standard transcript over root), p_random and
    p_eval, never on the columns"""
    bp = as_batch(proof)
    nl = O.limbs(bp.fid)
    tr = make_tr() if make_tr else O.standard_transcript(n_open, root)
    return B.replay_transcript(bp, np.asarray(bp.cols[0]).size // nl, n_open, tr)


@dataclass
class Ctx:
    """an honest proof with everything its mutations are built from"""
    fid: int
    p: int
    n_rows: int
    n_open: int
    root: bytes
    proof: "B.BatchProof"
    outers: list          # Montgomery arrays, one per evaluation
    inners: list
    o_enc: "O.Encoding"
    make_tr: Callable
    T: List[List[int]]    # the degree-test tensors, canonical
    U: List[List[int]]    # the outer tensors, canonical
    idx: List[int]
    tensors: list         # the degree-test tensors, Montgomery
    enc_random: list      # the encoded p_random vectors, (n_cols, limbs) each
    enc_evals: list       # the encoded p_eval vectors

    @property
    def ndt(self) -> int:
        return len(self.T)

    @property
    def m(self) -> int:
        return len(self.U)


def context(proof, root: bytes, outers, inners, o_enc, make_tr: Optional[Callable] = None) -> Ctx:
    bp = as_batch(proof)
    fid, nl, n_open = bp.fid, O.limbs(bp.fid), o_enc.n_col_opens
    make = make_tr or (lambda: O.standard_transcript(n_open, root))
    tensors, idx = replay(bp, root, n_open, make)
    n_rows = np.asarray(bp.cols[0]).size // nl

    def encode(v):
        row = np.zeros(bp.n_cols * nl, np.uint64)
        row[:np.asarray(v).size] = np.asarray(v, dtype=np.uint64).reshape(-1)
        return o_enc.encode(row).reshape(bp.n_cols, nl)

    return Ctx(fid, O.modulus(fid), n_rows, n_open, root, bp, list(outers), list(inners), o_enc, make,
               [canon(fid, t) for t in tensors], [canon(fid, u) for u in outers], [int(c) for c in idx],
               list(tensors), [encode(v) for v in bp.p_random], [encode(v) for v in bp.p_evals])


def column_verdict(ctx: Ctx, proof: "B.BatchProof", k: int, root: Optional[bytes] = None) -> int:
    """The oracle's verdict on a proof that differs from the honest one in opened column k alone (its
    words, its path) or in the root.  The oracle's verify loops over the opened columns and makes the
    same three checks on each, with the oracle functions called here (of_verify_column_value,
    of_verify_column_path); the tensors, the encoded vectors and the indices come from the transcript,
    which no column enters.  The columns before k are the honest proof's and pass, so column k's checks
    decide; if it passes too, so does the proof.  (The full verify of a 17-chunk proof costs 20 ms, a
    thousand mutations of it 20 s: test_verify_mut.py holds this shortcut to the full verify.)"""
    fid, lib = ctx.fid, O.lib()
    col = np.ascontiguousarray(proof.cols[k], dtype=np.uint64).reshape(-1)
    c = ctx.idx[k]

    def value(tensor, enc) -> bool:
        t = np.ascontiguousarray(tensor, dtype=np.uint64).reshape(-1)
        return bool(lib.of_verify_column_value(fid, O.p64(col), O.p64(t), ctx.n_rows, O.p64(np.ascontiguousarray(enc[c]))))

    if not all([value(t, e) for t, e in zip(ctx.tensors, ctx.enc_random)]):
        return COLUMN_DEGREE
    if not all([value(u, e) for u, e in zip(ctx.outers, ctx.enc_evals)]):
        return COLUMN_EVAL
    path = np.frombuffer(proof.paths[k], np.uint8)
    rp, keep = O.p8(ctx.root if root is None else root)
    if not lib.of_verify_column_path(fid, O.p64(col), ctx.n_rows, path.ctypes.data_as(O.u8p), len(proof.paths[k]) // 32,
                                     c, rp):
        return COLUMN_PATH
    return OK


def oracle_verdict(ctx: Ctx, proof: "B.BatchProof", root: Optional[bytes] = None, outers=None, inners=None):
    """(error kind, evaluations) from the oracle alone: the C verifier for one evaluation,
    batch_ref.verify_batch for several"""
    root = ctx.root if root is None else root
    outers = ctx.outers if outers is None else outers
    inners = ctx.inners if inners is None else inners
    if len(outers) == 1:
        rc, ev = as_oracle(proof, ctx.n_open).verify(root, outers[0], inners[0], ctx.o_enc, ctx.make_tr())
        return (rc + 9 if rc else OK), ([ev] if rc == 0 else None)
    return B.verify_batch(root, outers, inners, proof, ctx.o_enc, ctx.make_tr())


# ---------------------------------------------------------------- mutations
@dataclass
class Mutation:
    cls: str
    where: str
    proof: "B.BatchProof"
    root: bytes
    expect: Optional[int]      # the kind it was built for; None: the oracle decides
    aim: Optional[int] = None  # DEGREE_BLIND: the evaluation it fails
    k: Optional[int] = None    # the opened column it changes


def verdict(ctx: Ctx, mut: Mutation, full: bool = False):
    """(error kind, evaluations) of the oracle for a mutation: the full verify where the transcript
    moves or columns change places (and on request), column_verdict where one column or the root
    changed (the root meets column 0 first)"""
    if not full and mut.cls not in (EXCHANGE, P_EVAL, P_RANDOM):
        kind = column_verdict(ctx, mut.proof, 0 if mut.k is None else mut.k, mut.root)
        if kind != OK:
            return kind, None
    return oracle_verdict(ctx, mut.proof, root=mut.root)


def needs_rows(cls: str, ndt: int, m: int = 1) -> int:
    """rows a column class needs: the target and one helper per vector it is blind to"""
    return {RAW: 1, DEGREE_BLIND: ndt + m, ALL_BLIND: ndt + m + 1}[cls]


def column_delta(ctx: Ctx, cls: str, row: int, scale: int, aim: int = 0) -> List[int]:
    p = ctx.p
    if cls == RAW:
        delta = blind([], row, scale, ctx.n_rows, p)
        first = ctx.T[0] if ctx.T else ctx.U[0]   # what rejects it first
        assert dot(first, delta, p) != 0
    elif cls == DEGREE_BLIND:
        delta = blind(ctx.T + [u for j, u in enumerate(ctx.U) if j != aim], row, scale, ctx.n_rows, p)
        assert dot(ctx.U[aim], delta, p) != 0
        assert all(dot(u, delta, p) == 0 for j, u in enumerate(ctx.U) if j != aim)
    else:
        delta = blind(ctx.T + ctx.U, row, scale, ctx.n_rows, p)
        assert all(dot(v, delta, p) == 0 for v in ctx.T + ctx.U)
    return delta


def expected_kind(cls: str, ndt: int) -> int:
    if cls == RAW:
        return COLUMN_DEGREE if ndt else COLUMN_EVAL
    return COLUMN_EVAL if cls == DEGREE_BLIND else COLUMN_PATH


def with_column(bp: "B.BatchProof", k: int, col=None, path: Optional[bytes] = None) -> "B.BatchProof":
    cols, paths = list(bp.cols), list(bp.paths)
    if col is not None:
        cols[k] = col
    if path is not None:
        paths[k] = path
    return dataclasses.replace(bp, cols=cols, paths=paths)


def column_mutations(ctx: Ctx, ks: Sequence[int], rows: Sequence[int], scales: Sequence[int] = (1,),
                     classes: Sequence[str] = COLUMN_CLASSES, aims: Sequence[int] = (0,)) -> Iterator[Mutation]:
    """every class that the row count admits, at opened columns x rows x scales (DEGREE_BLIND once per
    aimed evaluation).  The deltas depend on (class, row, scale, aim) only and are shared by the columns."""
    for cls in classes:
        if ctx.n_rows < needs_rows(cls, ctx.ndt, ctx.m):
            continue
        for aim in (aims if cls == DEGREE_BLIND else (None,)):
            for row in rows:
                for scale in scales:
                    delta = column_delta(ctx, cls, row, scale, aim or 0)
                    for k in ks:
                        col = add_delta(ctx.fid, ctx.proof.cols[k], delta, ctx.p)
                        assert not np.array_equal(col, ctx.proof.cols[k])
                        yield Mutation(cls, f"col {k} row {row} scale 2^{scale.bit_length() - 1}"
                                       + (f" aim {aim}" if aim is not None else ""),
                                       with_column(ctx.proof, k, col=col), ctx.root, expected_kind(cls, ctx.ndt), aim, k)


def top_word_mutations(ctx: Ctx, ks: Sequence[int], rows: Sequence[int]) -> Iterator[Mutation]:
    """RAW with the one scale that moves the sum of the column's FIRST check (the first degree test; the
    evaluation when there is none) by exactly one unit of its top stored 32-bit word, so that sum and
    the encoded vector's entry differ in that word alone.  A comparison that leaves the top word out
    lets the column through to the next check, which reports another kind."""
    fid, p, nl = ctx.fid, ctx.p, O.limbs(ctx.fid)
    unit = 1 << (32 * (field_words(fid) - 1))
    vec, mont, enc = (ctx.T[0], ctx.tensors[0], ctx.enc_random[0]) if ctx.T else (ctx.U[0], ctx.outers[0], ctx.enc_evals[0])
    for k in ks:
        want = stored_int(fid, enc[ctx.idx[k]])
        moved = want + unit if want + unit < p else want - unit
        d = (canon(fid, O.limbs_from_ints([moved], nl))[0] - canon(fid, enc[ctx.idx[k]])[0]) % p
        for row in rows:
            delta = blind([], row, d * pow(vec[row], -1, p) % p, ctx.n_rows, p)
            col = add_delta(fid, ctx.proof.cols[k], delta, p)
            got = O.collapse(fid, col, np.ascontiguousarray(mont, dtype=np.uint64).reshape(-1), ctx.n_rows, 1)
            assert stored_int(fid, got) == moved and (stored_int(fid, got) ^ want) < unit << 32
            assert (stored_int(fid, got) ^ want) % unit == 0, "only the top word differs"
            yield Mutation(RAW_TOP, f"col {k} row {row}", with_column(ctx.proof, k, col=col), ctx.root,
                           expected_kind(RAW, ctx.ndt), None, k)


def n_column_mutations(n_rows: int, ndt: int, m: int, n_ks: int, n_row_places: int, n_scales: int = 1,
                       n_aims: int = 1) -> Dict[str, int]:
    """the count column_mutations must produce per class for a column of n_rows rows: everything,
    unless the column is too short for the class"""
    full = n_ks * n_row_places * n_scales
    return {cls: (full * (n_aims if cls == DEGREE_BLIND else 1) if n_rows >= needs_rows(cls, ndt, m) else 0)
            for cls in COLUMN_CLASSES}


def path_mutations(ctx: Ctx, ks: Sequence[int], byte_places: Sequence[int] = PATH_BYTES) -> Iterator[Mutation]:
    """one bit of a path digest, at opened columns x every level x bytes"""
    for k in ks:
        path = ctx.proof.paths[k]
        for level in range(len(path) // 32):
            for b in byte_places:
                yield Mutation(PATH, f"col {k} level {level} byte {b}",
                               with_column(ctx.proof, k, path=flip(path, 32 * level + b, k + level + b)),
                               ctx.root, COLUMN_PATH, None, k)


def root_mutations(ctx: Ctx) -> Iterator[Mutation]:
    """one bit of every root byte.  The transcript stays the honest one (the caller seeds it)."""
    for b in range(32):
        yield Mutation(ROOT, f"root byte {b}", ctx.proof, flip(ctx.root, b, b), COLUMN_PATH)


def exchange_mutations(ctx: Ctx) -> Iterator[Mutation]:
    """two opened columns exchanged, with and without their paths: positions with different column
    indices at a lane-group edge and, where the challenge drew one index twice, the two positions of
    that index.  The oracle decides."""
    pairs = []
    n = ctx.n_open
    a, b = (63, 64) if n > 64 else (0, n - 1)
    if ctx.idx[a] == ctx.idx[b]:
        b = next(k for k in range(n) if ctx.idx[k] != ctx.idx[a])
    pairs.append((a, b))
    seen = {}
    for k, c in enumerate(ctx.idx):
        if c in seen:
            pairs.append((seen[c], k))
            break
        seen[c] = k
    for a, b in pairs:
        for with_paths in (False, True):
            bp = with_column(with_column(ctx.proof, a, col=ctx.proof.cols[b],
                                         path=ctx.proof.paths[b] if with_paths else None),
                             b, col=ctx.proof.cols[a], path=ctx.proof.paths[a] if with_paths else None)
            yield Mutation(EXCHANGE, f"cols {a} <-> {b}" + (" with paths" if with_paths else ""), bp, ctx.root, None)


def vector_mutations(ctx: Ctx, n_per_row: int) -> Iterator[Mutation]:
    """an element of p_eval (every evaluation) or p_random (every degree test) replaced by another
    reduced one, at elements 0, 1 and the last.  The transcript moves with them: the oracle decides."""
    nl = O.limbs(ctx.fid)
    for cls, vecs in ((P_EVAL, ctx.proof.p_evals), (P_RANDOM, ctx.proof.p_random)):
        for j, vec in enumerate(vecs):
            for i in sorted({0, 1, n_per_row - 1}):
                v = np.array(vec, dtype=np.uint64, copy=True).reshape(-1)
                v[i * nl:(i + 1) * nl] = other_element(ctx.fid, v[i * nl:(i + 1) * nl], ctx.p)
                new = list(vecs)
                new[j] = v
                bp = dataclasses.replace(ctx.proof, **{"p_evals" if cls == P_EVAL else "p_random": new})
                yield Mutation(cls, f"vector {j} element {i}", bp, ctx.root, None)


# ---------------------------------------------------------------- the product's form
def product_columns(L, bp: "B.BatchProof"):
    nl = O.limbs(bp.fid)
    return [L.LcColumn(np.asarray(col, dtype=np.uint64).reshape(-1, nl), [p[i:i + 32] for i in range(0, len(p), 32)])
            for col, p in zip(bp.cols, bp.paths)]


def product_proof(L, bp: "B.BatchProof", batch: bool):
    """L.LcEvalProof / L.LcBatchEvalProof of the same words (L: the product package)"""
    if batch:
        return L.LcBatchEvalProof.from_parts(bp.fid, bp.n_cols, bp.p_evals, bp.p_random, product_columns(L, bp))
    return L.LcEvalProof.from_parts(bp.fid, bp.n_cols, bp.p_evals[0], bp.p_random, product_columns(L, bp))


def from_product(pf) -> "B.BatchProof":
    """a product proof (single or batch) as plain words"""
    cols = pf.columns
    evals = pf.p_eval_vec if hasattr(pf, "p_eval_vec") else [pf.p_eval]
    return B.BatchProof(pf.field, pf.n_cols, [v.reshape(-1) for v in evals], [v.reshape(-1) for v in pf.p_random_vec],
                        [], [c.col.reshape(-1) for c in cols], [b"".join(c.path) for c in cols])


# ---------------------------------------------------------------- the sweeps the tests share
def points(fid: int, n_per_row: int, n_rows: int, m: int, seed: int = 5):
    """m evaluation points: (inners, outers), Montgomery"""
    xs = O.ChaCha(seed_u64=seed + 31 * m + fid).field_random(fid, m).reshape(m, -1)
    pts = [O.eval_tensors(fid, xs[j], n_per_row, n_rows) for j in range(m)]
    return [p[0] for p in pts], [p[1] for p in pts]


def oracle_case(fid: int, shape: Shape, ndt: int, m: int = 1) -> dict:
    """coefficients, the oracle's encoding and commitment and m points for one shape"""
    coeffs = O.random_coeffs(fid, shape.n_rows * shape.n_per_row, 900 + 7 * fid + shape.n_rows)
    o_enc = O.Encoding.ligero(fid, shape.n_per_row, shape.n_cols, shape.n_open, ndt)
    o_comm = O.Commit(o_enc, coeffs)
    assert o_comm.n_rows == shape.n_rows
    inners, outers = points(fid, shape.n_per_row, shape.n_rows, m)
    return dict(fid=fid, shape=shape, ndt=ndt, m=m, coeffs=coeffs, o_enc=o_enc, o_comm=o_comm, root=o_comm.root(),
                inners=inners, outers=outers)


def oracle_context(case: dict) -> Ctx:
    """the oracle's own honest proof of a case (one evaluation: the C prover; several: batch_ref)"""
    tr = O.standard_transcript(case["shape"].n_open, case["root"])
    if case["m"] == 1:
        pf = as_batch(case["o_comm"].prove(case["o_enc"], case["outers"][0], tr))
    else:
        pf = B.prove_batch(case["o_comm"], case["o_enc"], case["outers"], tr)
    return context(pf, case["root"], case["outers"], case["inners"], case["o_enc"])


def word_columns(ks: Sequence[int]) -> List[int]:
    """the two opened columns of the word sweep: the first, and the first lane of the second group
    (the last opened column when there is no second group)"""
    return sorted({ks[0], 64 if 64 in ks else ks[-1]})


def sweep(ctx: Ctx, shape: Shape) -> Iterator[Mutation]:
    """every mutation of one proof (single or batch): the column classes at opened columns x rows with
    scale 1 (DEGREE_BLIND aimed at every evaluation in turn), every 32-bit word at one row per chunk of
    two opened columns, the top-stored-word change of the first check at those two, the path levels, the root bytes, exchanged columns, changed vectors"""
    ks = opened_places(ctx.n_open, ctx.ndt + ctx.m)
    aims = range(ctx.m)
    yield from column_mutations(ctx, ks, row_places(ctx.fid, ctx.n_rows, shape.thin_rows), aims=aims)
    yield from column_mutations(ctx, word_columns(ks), word_rows(ctx.fid, ctx.n_rows), word_scales(ctx.fid)[1:],
                                aims=aims)
    yield from top_word_mutations(ctx, word_columns(ks), word_rows(ctx.fid, ctx.n_rows)[-1:])
    yield from path_mutations(ctx, ks)
    yield from root_mutations(ctx)
    yield from exchange_mutations(ctx)
    yield from vector_mutations(ctx, shape.n_per_row)


def sweep_counts(fid: int, shape: Shape, ndt: int, m: int = 1) -> Dict[str, int]:
    """what sweep must produce per class, from the place lists alone; EXCHANGE is at least 2 (two more
    when the challenge drew a column twice)"""
    ks = opened_places(shape.n_open, ndt + m)
    a = n_column_mutations(shape.n_rows, ndt, m, len(ks), len(row_places(fid, shape.n_rows, shape.thin_rows)), 1, m)
    b = n_column_mutations(shape.n_rows, ndt, m, len(word_columns(ks)), len(word_rows(fid, shape.n_rows)),
                           field_words(fid) - 1, m)
    out = {cls: a[cls] + b[cls] for cls in COLUMN_CLASSES}
    n_elems = len({0, 1, shape.n_per_row - 1})
    path_len = max(shape.n_cols - 1, 0).bit_length()
    out.update({RAW_TOP: len(word_columns(ks)), PATH: len(ks) * path_len * len(PATH_BYTES), ROOT: 32,
                P_EVAL: m * n_elems, P_RANDOM: ndt * n_elems})
    return out
