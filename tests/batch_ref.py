"""Reference for batched evaluation proofs (checker only): the prover and verifier of
lcpc-2d/src/lib.rs:862-982 and :1034-1123 restated in Python over the oracle's primitives
(oracle_ffi: Transcript, ChaCha.field_random, ChaCha.uniform, collapse, Encoding.encode, Commit,
verify_path), widened from one outer tensor to m:

  1. the degree tests as in prove (challenge tensor under "$l//DT", row combination, every
     coefficient absorbed under "$l//PR");
  2. p_eval_0 .. p_eval_(m-1) = the row combinations with the m outer tensors, absorbed in order,
     every coefficient under "$l//PE";
  3. the column challenge under "$l//CO", the opened columns and their Merkle paths.

With m = 1 this is the reference's prove / verify (test_batch_ref.py pins it to the oracle's own
Commit.prove part for part)."""
import struct
from dataclasses import dataclass
from typing import List

import numpy as np

import oracle_ffi as O

# VerifierError kinds (include/lcpc_mi.h)
OK, NUM_COL_OPENS, COLUMN_PATH, COLUMN_EVAL, COLUMN_DEGREE, OUTER_TENSOR, INNER_TENSOR = 0, 10, 11, 12, 13, 14, 15
FT253_192 = 4  # the one field whose repr is big-endian


def repr_bytes(fid: int, elems: np.ndarray) -> List[bytes]:
    """PrimeField::to_repr of each Montgomery element: canonical bytes (little-endian limbs;
    Ft253_192 big-endian)"""
    nl = O.limbs(fid)
    a = np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1)
    can = np.zeros_like(a)
    O.lib().of_to_canonical(fid, O.p64(a), O.p64(can), a.size // nl)
    raw = can.astype("<u8").tobytes()
    w = 8 * nl
    out = [raw[i:i + w] for i in range(0, len(raw), w)]
    return [b[::-1] for b in out] if fid == FT253_192 else out


def absorb(tr, label: bytes, fid: int, elems: np.ndarray):
    for b in repr_bytes(fid, elems):
        tr.append_message(label, b)


def challenge_tensor(tr, fid: int, n_rows: int) -> np.ndarray:
    return O.ChaCha(seed=tr.challenge_bytes(O.LABEL["DT"], 32)).field_random(fid, n_rows)


def challenge_columns(tr, n_cols: int, n_col_opens: int) -> List[int]:
    rng = O.ChaCha(seed=tr.challenge_bytes(O.LABEL["CO"], 32))
    return [rng.uniform(0, n_cols) for _ in range(n_col_opens)]


def log2_np2(n: int) -> int:
    return max(n - 1, 0).bit_length()


@dataclass
class BatchProof:
    fid: int
    n_cols: int
    p_evals: List[np.ndarray]   # m vectors of n_per_row * limbs words
    p_random: List[np.ndarray]  # n_degree_tests vectors
    col_idx: List[int]
    cols: List[np.ndarray]      # n_col_opens columns of n_rows * limbs words
    paths: List[bytes]          # n_col_opens paths of path_len * 32 bytes


def open_columns(comm: "O.Commit", idx: List[int]):
    """the columns idx of the encoded matrix and their Merkle paths (open_column, lib.rs:818-855)"""
    nr, nc, nl = comm.n_rows, comm.n_cols, comm.nl
    cm = comm.comm.reshape(nr, nc, nl)
    hashes = comm.hashes
    np2, pl = 1 << log2_np2(nc), log2_np2(nc)
    cols, paths = [], []
    for c in idx:
        cols.append(np.ascontiguousarray(cm[:, c, :]).reshape(-1))
        path, off, width, i = [], 0, np2, c
        for _ in range(pl):
            sib = off + (i ^ 1)
            path.append(hashes[32 * sib:32 * sib + 32])
            off += width
            width >>= 1
            i >>= 1
        paths.append(b"".join(path))
    return cols, paths


def replay_transcript(pf: "BatchProof", n_rows: int, n_col_opens: int, tr):
    """the verifier's Fiat-Shamir pass over a proof's vectors: (degree-test tensors, column indices)"""
    tensors = []
    for pr in pf.p_random:
        tensors.append(challenge_tensor(tr, pf.fid, n_rows))
        absorb(tr, O.LABEL["PR"], pf.fid, pr)
    for pe in pf.p_evals:
        absorb(tr, O.LABEL["PE"], pf.fid, pe)
    return tensors, challenge_columns(tr, pf.n_cols, n_col_opens)


def reopen(comm: "O.Commit", enc: "O.Encoding", pf: "BatchProof", tr) -> "BatchProof":
    """A forger's best follow-up to changed p_random / p_eval vectors: the changed vectors redraw the
    column challenge, so the columns are opened again, honestly, where the new challenge falls.
    (A forgery that keeps the old columns presents them at the wrong indices and already fails the
    first per-column check, ColumnDegree.)"""
    _, idx = replay_transcript(pf, comm.n_rows, enc.n_col_opens, tr)
    cols, paths = open_columns(comm, idx)
    return BatchProof(pf.fid, pf.n_cols, pf.p_evals, pf.p_random, idx, cols, paths)


def prove_batch(comm: "O.Commit", enc: "O.Encoding", outers: List[np.ndarray], tr) -> BatchProof:
    fid, nl = comm.fid, comm.nl
    nr, npr, nc = comm.n_rows, comm.n_per_row, comm.n_cols
    coeffs = comm.coeffs
    p_random = []
    for _ in range(enc.n_degree_tests):
        t = challenge_tensor(tr, fid, nr)
        pr = O.collapse(fid, coeffs, t, nr, npr)
        absorb(tr, O.LABEL["PR"], fid, pr)
        p_random.append(pr)
    p_evals = [O.collapse(fid, coeffs, np.ascontiguousarray(o, dtype=np.uint64).reshape(-1), nr, npr)
               for o in outers]
    for pe in p_evals:
        absorb(tr, O.LABEL["PE"], fid, pe)
    idx = challenge_columns(tr, nc, enc.n_col_opens)
    cols, paths = open_columns(comm, idx)
    return BatchProof(fid, nc, p_evals, p_random, idx, cols, paths)


def _dot(fid: int, a: np.ndarray, b: np.ndarray, n: int) -> np.ndarray:
    """sum_i a[i] b[i] as a collapse of the n x 1 matrix a by the tensor b"""
    return O.collapse(fid, np.ascontiguousarray(a, dtype=np.uint64).reshape(-1),
                      np.ascontiguousarray(b, dtype=np.uint64).reshape(-1), n, 1)


def verify_batch(root: bytes, outers, inners, pf: BatchProof, enc: "O.Encoding", tr):
    """(error kind, evaluations): per opened column ColumnDegree, then ColumnEval (any j), then
    ColumnPath, as verify's loop (lib.rs:953-974) orders them."""
    fid, nl = pf.fid, O.limbs(pf.fid)
    m = len(outers)
    if len(pf.cols) != enc.n_col_opens or enc.n_col_opens == 0:
        return NUM_COL_OPENS, None
    npr, nc = pf.p_evals[0].size // nl, pf.n_cols
    nr = pf.cols[0].size // nl
    if any(np.asarray(i).size // nl != npr for i in inners):
        return INNER_TENSOR, None
    if any(np.asarray(o).size // nl != nr for o in outers) or len(pf.p_evals) != m:
        return OUTER_TENSOR, None
    tensors, idx = replay_transcript(pf, nr, enc.n_col_opens, tr)

    def encode(v):
        row = np.zeros(nc * nl, np.uint64)
        row[:npr * nl] = v
        return enc.encode(row).reshape(nc, nl)

    enc_random = [encode(v) for v in pf.p_random]
    enc_evals = [encode(v) for v in pf.p_evals]
    for k, c in enumerate(idx):
        col = pf.cols[k]
        for t, e in zip(tensors, enc_random):
            if not np.array_equal(_dot(fid, col, t, nr), e[c]):
                return COLUMN_DEGREE, None
        for o, e in zip(outers, enc_evals):
            if not np.array_equal(_dot(fid, col, o, nr), e[c]):
                return COLUMN_EVAL, None
        leaf = O.hash_columns(fid, col, nr, 1)
        if not O.verify_path(leaf, c, pf.paths[k], root):
            return COLUMN_PATH, None
    return OK, [_dot(fid, pe, i, npr) for pe, i in zip(pf.p_evals, inners)]


# ---- the byte layout of LcBatchEvalProof.to_bytes: LcEvalProof's bincode form
# with p_eval widened to a length-prefixed vector of vectors
def _vec_f(a, nl: int) -> bytes:
    a = np.ascontiguousarray(a, dtype="<u8").reshape(-1, nl)
    return struct.pack("<Q", a.shape[0]) + a.tobytes()


def to_bytes(pf: BatchProof) -> bytes:
    nl, q = O.limbs(pf.fid), struct.Struct("<Q").pack
    parts = [q(pf.n_cols), q(len(pf.p_evals))] + [_vec_f(x, nl) for x in pf.p_evals]
    parts += [q(len(pf.p_random))] + [_vec_f(x, nl) for x in pf.p_random]
    parts.append(q(len(pf.cols)))
    for col, path in zip(pf.cols, pf.paths):
        parts += [_vec_f(col, nl), q(len(path) // 32)]
        parts += [q(32) + path[i:i + 32] for i in range(0, len(path), 32)]
    return b"".join(parts)


def from_bytes(fid: int, data: bytes) -> BatchProof:
    """col_idx is not part of the bytes (the verifier redraws it): left empty"""
    nl, off = O.limbs(fid), 0

    def u64():
        nonlocal off
        if off + 8 > len(data):
            raise ValueError("truncated")
        v = struct.unpack_from("<Q", data, off)[0]
        off += 8
        return v

    def vec_f():
        nonlocal off
        n = u64()
        if off + 8 * n * nl > len(data):
            raise ValueError("truncated")
        a = np.frombuffer(data, "<u8", n * nl, off).astype(np.uint64)
        off += 8 * n * nl
        return a

    n_cols = u64()
    p_evals = [vec_f() for _ in range(u64())]
    p_random = [vec_f() for _ in range(u64())]
    cols, paths = [], []
    for _ in range(u64()):
        cols.append(vec_f())
        path = []
        for _ in range(u64()):
            if u64() != 32 or off + 32 > len(data):
                raise ValueError("digest")
            path.append(data[off:off + 32])
            off += 32
        paths.append(b"".join(path))
    if off != len(data):
        raise ValueError("trailing bytes")
    return BatchProof(fid, n_cols, p_evals, p_random, [], cols, paths)
