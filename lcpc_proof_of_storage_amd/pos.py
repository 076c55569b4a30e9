"""proof-of-storage producers of the commitment path, restated over liblcpc_mi.so.

Mirrors the functions of the reference's proof-of-storage crate that feed / consume the lcpc-2d
commitment (names kept):
  fields::convert_byte_vec_to_field_elements_vec        fields.rs:109-112, data_field.rs:38-46
  fields::convert_field_elements_vec_to_byte_vec        fields.rs:114-121
  fields::field_generator_iter::FieldGeneratorIter      fields/field_generator_iter.rs:5-55
  fields::{read_file_to_field_elements_vec, stream_file_to_field_elements_vec_sync,
           read_file_path_to_field_elements_vec, field_elements_vec_to_file,
           random_writeable_field_vec, evaluate_field_polynomial_at_point[_with_elevated_degree],
           vector_multiply, is_power_of_two}          fields.rs:25-194
  lcpc_online::dims_ok                                   lcpc_online.rs:71-76
  networking::server::get_aspect_ratio_default_from_field_len / _from_file_len
                                                         networking/server.rs:1139-1182
  networking::client::get_column_indicies_from_random_seed   networking/client.rs:443-456
  lcpc_online::{convert_file_data_to_commit, verifiable_polynomial_evaluation, decode_row,
                form_side_vectors_for_polynomial_evaluation_from_point,
                server_retreive_columns, hash_column_to_digest,
                client_online_verify_column_paths[_without_full_columns],
                client_online_verify_column_leaves, client_verify_commitment[_without_full_columns],
                hash_column_to_digest, hash_field_vec_to_digest, _get_POS_soundness_n_cols,
                verify_proper_partial_polynomial_evaluation, verifiable_full_polynomial_evaluation,
                verify_full_polynomial_evaluation_wrapper_with_single_eval_point}
                                                         lcpc_online.rs:80-627
  lcpc_online::file_handler::left_multiply_unencoded_matrix_by_vector   file_handler.rs:614-638
The field is WriteableFt63: the modulus, arithmetic and repr of FT63.

Without a counterpart in the reference: the update audits' client checks and the
checkable read, read_plan / ReadOpening / client_verify_read (§5e).
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .lcpc2d import (FT63, VERIFIER, DeviceError, LcColumn, LcCommit, LigeroEncoding, ProverError, VerifierError,
                     _p64, _raise, collapse_columns, collapse_columns_many, digest_name, limbs, verify_column_path)

WRITTEN_BYTES_WIDTH = 8   # size_of::<WriteableFt63>() (data_field.rs:24)
DATA_BYTE_CAPACITY = 7    # CAPACITY / 8 (data_field.rs:22)


def _u8p(b: bytes):
    buf = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")
    return C.cast(buf, N.u8p), buf


def convert_byte_vec_to_field_elements_vec(data: bytes) -> np.ndarray:
    """7 LE bytes per element, raw limb (WriteableFt63::from_data_bytes); shape (n, 1)."""
    n = (len(data) + 6) // 7
    out = np.zeros((n, 1), np.uint64)
    p, keep = _u8p(data)
    got = C.c_size_t()
    _raise(N.load().lcpc_pos_bytes_to_field(p, len(data), _p64(out), C.byref(got)))
    return out


def convert_field_elements_vec_to_byte_vec(elems: np.ndarray, expected_length: int) -> bytes:
    a = np.ascontiguousarray(elems, dtype=np.uint64).reshape(-1)
    out = (C.c_uint8 * max(expected_length, 1))()
    _raise(N.load().lcpc_pos_field_to_bytes(_p64(a), a.size, C.cast(out, N.u8p), expected_length))
    return bytes(out)[:expected_length]


class FieldGeneratorIter:
    """FieldGeneratorIter<I, WriteableFt63> (fields/field_generator_iter.rs:5-55): an iterator of
    bytes (ints 0..255, or bytes-like blocks) to field elements, DATA_BYTE_CAPACITY = 7 bytes each,
    the last one zero padded -- the elements convert_byte_vec_to_field_elements_vec gives for the
    same bytes.  Bytes are packed a block at a time by the library (lcpc_pos_bytes_to_field);
    elements come out as uint64 raw limbs.  `byte_blocks()` hands a consumer the remaining bytes
    themselves in blocks of whole elements (RowGeneratorIter's digest path)."""

    BLOCK = DATA_BYTE_CAPACITY * 65536

    def __init__(self, inner):
        if isinstance(inner, (bytes, bytearray, memoryview)):
            mv = memoryview(inner).cast("B")
            inner = (bytes(mv[i:i + self.BLOCK]) for i in range(0, len(mv), self.BLOCK))
        self._inner = iter(inner)
        self._carry = b""          # bytes read but not yet packed (fewer than a whole block)
        self._elems = np.zeros(0, np.uint64)
        self._pos = 0
        self._done = False

    def _read(self, want: int) -> bytes:
        """Up to `want` bytes (fewer only at the end of the input)."""
        parts, have = [self._carry], len(self._carry)
        while have < want and not self._done:
            try:
                x = next(self._inner)
            except StopIteration:
                self._done = True
                break
            b = bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else bytes((x,))
            parts.append(b)
            have += len(b)
        buf = b"".join(parts)
        self._carry = buf[want:]
        return buf[:want]

    def __iter__(self):
        return self

    def __next__(self) -> np.uint64:
        if self._pos == self._elems.size:
            block = self._read(self.BLOCK)
            if not block:
                raise StopIteration
            self._elems = convert_byte_vec_to_field_elements_vec(block).reshape(-1)
            self._pos = 0
        v = self._elems[self._pos]
        self._pos += 1
        return v

    def byte_blocks(self):
        """The rest of the input as bytes: first the elements already packed but not yet taken
        (7 little-endian bytes each), then the unread bytes in blocks."""
        if self._pos < self._elems.size:
            rest = self._elems[self._pos:]
            self._pos = self._elems.size
            yield rest.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :DATA_BYTE_CAPACITY].tobytes()
        while True:
            block = self._read(self.BLOCK)
            if not block:
                return
            yield block


def read_file_to_field_elements_vec(file) -> tuple:
    """fields.rs:25-35: (bytes read, elements) of a whole binary file object."""
    data = file.read()
    return len(data), convert_byte_vec_to_field_elements_vec(data)


def stream_file_to_field_elements_vec_sync(file) -> tuple:
    """fields.rs:72-106: the same elements, read in buffers of 1000 whole elements (7000 bytes,
    the reference's BufReader size), each buffer packed by the library.  (file size, elements)."""
    buf = 1000 * DATA_BYTE_CAPACITY
    parts, total = [], 0
    while True:
        b = file.read(buf)
        if not b:
            break
        total += len(b)
        parts.append(convert_byte_vec_to_field_elements_vec(b))
    return total, (np.concatenate(parts) if parts else np.zeros((0, 1), np.uint64))


def read_file_path_to_field_elements_vec(path: str) -> np.ndarray:
    """fields.rs:122-127."""
    with open(path, "rb") as f:
        return read_file_to_field_elements_vec(f)[1]


def field_elements_vec_to_file(path: str, field_elements) -> None:
    """fields.rs:129-146: each element's 7 data bytes in turn; the last element's trailing zero
    bytes are dropped (an empty vector gives an empty file)."""
    a = np.ascontiguousarray(field_elements, dtype=np.uint64).reshape(-1)
    data = convert_field_elements_vec_to_byte_vec(a, a.size * DATA_BYTE_CAPACITY) if a.size else b""
    if a.size:
        head, last = data[:-DATA_BYTE_CAPACITY], data[-DATA_BYTE_CAPACITY:].rstrip(b"\0")
        data = head + last
    with open(path, "wb") as f:
        f.write(data)


def random_writeable_field_vec(log_len: int, seed: int = 0) -> np.ndarray:
    """fields.rs:148-158: 7 * 2^log_len random bytes packed to 2^log_len elements (the
    reference draws them from a thread RNG; here a seeded one)."""
    data = np.random.default_rng(seed).integers(0, 256, DATA_BYTE_CAPACITY << log_len, dtype=np.uint8).tobytes()
    return convert_byte_vec_to_field_elements_vec(data)


def is_power_of_two(x: int) -> bool:
    """fields.rs:192-194 (true for 0, as x & (x - 1) is)."""
    return x & (x - 1) == 0 if x else True


def dims_ok(num_pre_encoded_columns: int, num_encoded_columns: int) -> bool:
    """lcpc_online.rs:71-76: a power-of-two width >= 2, >= 1 column, rate at most 1/2."""
    return (num_encoded_columns > 0 and num_encoded_columns & (num_encoded_columns - 1) == 0
            and num_pre_encoded_columns >= 1 and num_encoded_columns >= 2
            and num_encoded_columns >= 2 * num_pre_encoded_columns)


def get_aspect_ratio_default_from_field_len(field_len: int):
    """(num_pre_encoded_columns, num_encoded_matrix_columns, soundness)."""
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    N.load().lcpc_pos_default_dims(field_len, C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def get_aspect_ratio_default_from_file_len(file_len: int):
    return get_aspect_ratio_default_from_field_len(-(-file_len // WRITTEN_BYTES_WIDTH))


def get_column_indicies_from_random_seed(random_seed: int, number_of_columns_to_extract: int,
                                         max_column_index: int) -> List[int]:
    out = np.zeros(max(number_of_columns_to_extract, 1), np.uint64)
    n = C.c_size_t()
    _raise(N.load().lcpc_pos_column_indices(random_seed, number_of_columns_to_extract, max_column_index,
                                            _p64(out), C.byref(n)))
    return [int(v) for v in out[:n.value]]


def form_side_vectors_for_polynomial_evaluation_from_point(evaluation_point: np.ndarray, n_rows: int,
                                                           n_cols: int, field: int = FT63):
    """(left, right): left = [1, x^n_cols, ...] (n_rows), right = [1, x, ...] (n_cols)."""
    nl = limbs(field)
    x = np.ascontiguousarray(evaluation_point, dtype=np.uint64).reshape(-1)[:nl].copy()
    left = np.zeros((max(n_rows, 1), nl), np.uint64)
    right = np.zeros((max(n_cols, 1), nl), np.uint64)
    _raise(N.load().lcpc_pos_side_vectors(field, _p64(x), n_rows, n_cols, _p64(left), _p64(right)))
    return left[:n_rows], right[:n_cols]


def verifiable_polynomial_evaluation(commitment: LcCommit, left_evaluation_column) -> np.ndarray:
    """u^T Enc(M): n_cols results over the encoded matrix (lcpc_online.rs:454-484)."""
    u = np.ascontiguousarray(left_evaluation_column, dtype=np.uint64).reshape(-1, limbs(commitment.field))
    out = np.zeros((commitment.get_n_cols(), limbs(commitment.field)), np.uint64)
    _raise(N.load().lcpc_pos_eval_encoded(commitment._h, _p64(u), u.shape[0], _p64(out)))
    return out


def ifft_oi_rows(rows: np.ndarray, field: int = FT63) -> np.ndarray:
    """fffft::ifft_oi on every row of a (n_rows, len, limbs) or (len, limbs) array."""
    nl = limbs(field)
    a = np.ascontiguousarray(rows, dtype=np.uint64).copy()
    shape = a.shape
    a2 = a.reshape(-1, (a.size // nl) if a.ndim <= 2 else shape[-2] * nl)
    length = a2.shape[1] // nl
    _raise(N.load().lcpc_ifft_oi_rows(field, _p64(a2), a2.shape[0], length))
    return a2.reshape(shape)


def decode_row(row: np.ndarray, field: int = FT63) -> np.ndarray:
    """lcpc_online::decode_row = ifft_oi (lcpc_online.rs:568-574)."""
    return ifft_oi_rows(row, field)


# ---------------------------------------------------------------- R-S erasure decoding
# No counterpart in the reference (include/lcpc_mi.h, "R-S erasure decoding, scrub, repair").
UNRECOVERABLE = 36  # LCPC_ERR_UNRECOVERABLE


def rs_domain_points(field: int, length: int) -> np.ndarray:
    """The evaluation points of an encoded row in codeword order, (length, limbs) Montgomery limbs:
    position c of a codeword of f is f(points[c]).  Host only."""
    out = np.zeros((max(length, 1), limbs(field)), np.uint64)
    _raise(N.load().lcpc_rs_domain_points(field, length, _p64(out)))
    return out[:length]


def erasure_decode_rows(field: int, rows: np.ndarray, n_per_row: int, erased) -> np.ndarray:
    """rows: (n_rows, len, limbs) or (len, limbs) codewords of messages of n_per_row coefficients
    whose positions `erased` are unknown (never read).  Returns a copy with those positions filled
    in; every other limb is the input's.  At most len - n_per_row erasures; with fewer, rows that
    are no codeword on their surviving positions raise (code UNRECOVERABLE), as too many erasures
    do.  An empty `erased` is that consistency check alone."""
    nl = limbs(field)
    a = np.ascontiguousarray(rows, dtype=np.uint64).copy()
    shape = a.shape
    length = shape[-2] if a.ndim >= 2 else a.size // nl
    a2 = a.reshape(-1, length * nl)
    e = np.ascontiguousarray(np.asarray(list(erased), dtype=np.uint64).reshape(-1))
    _raise(N.load().lcpc_rs_erasure_decode_rows(field, _p64(a2), a2.shape[0], length, n_per_row,
                                                _p64(e) if e.size else None, e.size))
    return a2.reshape(shape)


def rs_locate_max_errors(field: int) -> int:
    """The most wrong positions per row the locator can name for this field (at least 256)."""
    return int(N.load().lcpc_rs_locate_max_errors(field))


def _rows_and_erasures(field: int, rows, erased):
    nl = limbs(field)
    a = np.ascontiguousarray(rows, dtype=np.uint64).copy()
    shape = a.shape
    length = shape[-2] if a.ndim >= 2 else a.size // nl
    a2 = a.reshape(-1, length * nl)
    e = np.ascontiguousarray(np.asarray(list(erased), dtype=np.uint64).reshape(-1))
    return a2, shape, length, e


def locate_errors_rows(field: int, rows: np.ndarray, n_per_row: int, erased=()):
    """Which positions of each row are wrong, from the row alone (syndromes, Berlekamp-Massey, root
    search).  rows as erasure_decode_rows; the positions `erased` are known to be missing and never
    read.  Returns (row_status, row_n_errors, err_mask, col_any): row_status[r] = 0 the row is a
    codeword on its surviving positions, 1 its wrong positions are located (err_mask[r, c] = 1
    there), 2 not locatable: more than (len - n_per_row - len(erased)) // 2 of them, or more than
    rs_locate_max_errors(field).  col_any[c] = 1 if any located row names position c."""
    a2, _, length, e = _rows_and_erasures(field, rows, erased)
    n = a2.shape[0]
    status = np.zeros(max(n, 1), np.uint8)
    n_err = np.zeros(max(n, 1), np.uint32)
    mask = np.zeros((max(n, 1), length), np.uint8)
    col_any = np.zeros(length, np.uint8)
    _raise(N.load().lcpc_rs_locate_errors_rows(
        field, _p64(a2), n, length, n_per_row, _p64(e) if e.size else None, e.size,
        status.ctypes.data_as(N.u8p), n_err.ctypes.data_as(N.u32p), mask.ctypes.data_as(N.u8p),
        col_any.ctypes.data_as(N.u8p)))
    return status[:n], n_err[:n], mask[:n], col_any


def decode_rows(field: int, rows: np.ndarray, n_per_row: int, erased=()) -> np.ndarray:
    """Errors-and-erasures correction: a copy of rows with the erased and the located wrong positions
    holding the codeword's values; every other limb is the input's.  Raises (code UNRECOVERABLE)
    if any row is not locatable; nothing is corrected then."""
    a2, shape, length, e = _rows_and_erasures(field, rows, erased)
    _raise(N.load().lcpc_rs_decode_rows(field, _p64(a2), a2.shape[0], length, n_per_row,
                                        _p64(e) if e.size else None, e.size, None))
    return a2.reshape(shape)


# ---------------------------------------------------------------- convert_file_data_to_commit
@dataclass
class Commit:
    pass


@dataclass
class Leaves:
    columns: Sequence[int]


@dataclass
class ColumnsWithPath:
    columns: Sequence[int]


@dataclass
class ColumnsWithoutPath:
    columns: Sequence[int]


@dataclass
class Specified:
    num_pre_encoded_columns: int
    num_encoded_columns: int


class Square:
    pass


def commit_dimensions(data_len: int, dims) -> tuple:
    """The (num_pre_encoded_columns, num_encoded_columns) of convert_file_data_to_commit
    (lcpc_online.rs:91-132), with its `ensure!` checks as ProverError(Commit)."""
    if data_len <= 0:
        raise ValueError("Cannot convert empty file to commit")
    if isinstance(dims, Specified):
        np_, nc = dims.num_pre_encoded_columns, dims.num_encoded_columns
        if np_ < 1 or nc < 2 or nc & (nc - 1) or not nc > np_:
            raise ValueError(f"bad commit dimensions {np_}/{nc}")
        return np_, nc
    w = math.ceil(float(np.sqrt(np.float32(data_len))))  # (data_len as f32).sqrt().ceil()
    np_ = w if (w & (w - 1)) == 0 else 1 << (w - 1).bit_length()
    nc = 1 << np_.bit_length()  # (np + 1).next_power_of_two()
    return np_, nc


def convert_file_data_to_commit(field_data: np.ndarray, what_to_extract, dimensions):
    """Commit -> LcCommit; Leaves -> list of 32-byte digests; ColumnsWithPath -> [LcColumn];
    ColumnsWithoutPath -> (n, n_rows, limbs) array."""
    data = np.ascontiguousarray(field_data, dtype=np.uint64).reshape(-1, limbs(FT63))
    np_, nc = commit_dimensions(data.shape[0], dimensions)
    enc = LigeroEncoding.new_from_dims(FT63, np_, nc)
    if isinstance(what_to_extract, Commit):
        return LcCommit.commit(data, enc)
    if isinstance(what_to_extract, ColumnsWithPath):
        comm = LcCommit.commit(data, enc)
        return comm.open_columns(list(what_to_extract.columns))
    idx = np.ascontiguousarray(list(what_to_extract.columns), dtype=np.uint64)
    n_rows = -(-data.shape[0] // np_)
    nl = limbs(FT63)
    cols = np.zeros((max(len(idx), 1), n_rows, nl), np.uint64)
    leaves = (C.c_uint8 * max(32 * len(idx), 1))()
    want_leaves = isinstance(what_to_extract, Leaves)
    _raise(N.load().lcpc_pos_columns(enc._h, _p64(data), data.shape[0], _p64(idx) if len(idx) else None,
                                     len(idx), _p64(cols),
                                     C.cast(leaves, N.u8p) if want_leaves else None))
    if want_leaves:
        b = bytes(leaves)
        return [b[32 * i:32 * i + 32] for i in range(len(idx))]
    return cols[:len(idx)]


def vector_multiply(a, b, field: int = FT63) -> np.ndarray:
    """fields.rs:188-190 = field_dot."""
    return field_dot(a, b, field)


def evaluate_field_polynomial_at_point_with_elevated_degree(field_elements, point, degree_offset: int,
                                                            field: int = FT63) -> np.ndarray:
    """fields.rs:172-186: sum_i c_i x^(i + degree_offset), one streaming pass on the GPU
    (lcpc_eval_poly: no power vector is formed)."""
    nl = limbs(field)
    c = np.ascontiguousarray(field_elements, dtype=np.uint64).reshape(-1, nl)
    x = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1)[:nl].copy()
    out = np.zeros((1, nl), np.uint64)
    _raise(N.load().lcpc_eval_poly(field, _p64(c) if c.size else None, c.shape[0], _p64(x), degree_offset, _p64(out)))
    return out


def evaluate_field_polynomial_at_point(field_elements, point, field: int = FT63) -> np.ndarray:
    """fields.rs:160-170: sum_i c_i x^i (coefficients little-endian: c_0 first)."""
    return evaluate_field_polynomial_at_point_with_elevated_degree(field_elements, point, 0, field)


def evaluate_bytes_polynomial_at_point(data, point, degree_offset: int = 0) -> np.ndarray:
    """The same over convert_byte_vec_to_field_elements_vec(data), read straight from the bytes
    (lcpc_pos_eval_poly_bytes; bytes-like or a uint8 array of any alignment)."""
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    x = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1)[:1].copy()
    out = np.zeros((1, 1), np.uint64)
    _raise(N.load().lcpc_pos_eval_poly_bytes(a.ctypes.data if a.size else None, a.size, _p64(x), degree_offset,
                                             _p64(out)))
    return out


def server_retreive_columns(comm: LcCommit, requested_columns: Sequence[int]) -> List[LcColumn]:
    return comm.open_columns(list(requested_columns))


def field_dot(a, b, field: int = FT63) -> np.ndarray:
    """fields::vector_multiply (fields.rs): sum_i a[i] b[i], on the GPU (a one-column collapse)."""
    nl = limbs(field)
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.uint64).reshape(-1))
    n = min(a.size, b.size) // nl
    if n == 0:
        return np.zeros((1, nl), np.uint64)
    return collapse_columns(field, a[:n * nl], b[:n * nl], n, 1)


def _verifier_error(kind: str, msg: str) -> VerifierError:
    code = {v: k for k, v in VERIFIER.items()}[kind]
    return VerifierError(code, msg)


def client_online_verify_column_paths(root: bytes, requested_columns: Sequence[int],
                                      received_columns: Sequence[LcColumn], field: int = FT63) -> None:
    """lcpc_online.rs:251-277: every received column's Merkle path leads to root.
    Raises VerifierError(ColumnEval) otherwise, as the reference's Err."""
    if len(requested_columns) != len(received_columns):
        raise _verifier_error("ColumnEval", "column count")
    if not received_columns:
        return
    leaves = hash_columns_to_digests(received_columns, field)
    client_online_verify_column_paths_without_full_columns(
        root, requested_columns, leaves, [c.path for c in received_columns])


def client_online_verify_column_paths_without_full_columns(
        root: bytes, requested_columns: Sequence[int], received_columns_digests: Sequence[bytes],
        received_column_paths: Sequence[Sequence[bytes]]) -> None:
    """lcpc_online.rs:280-318 (the paths checked on the GPU in one launch)."""
    n = len(requested_columns)
    if len(received_column_paths) != n or len(received_columns_digests) < n:
        raise _verifier_error("ColumnEval", "column count")
    if n == 0:
        return
    plen = len(received_column_paths[0])
    if any(len(p) != plen for p in received_column_paths):
        raise _verifier_error("ColumnEval", "path lengths differ")
    # untrusted server data: every digest is exactly one BLAKE3 output (the reference's
    # Output<Blake3> is a fixed 32-byte array, so anything else never deserializes)
    if any(len(d) != 32 for d in received_columns_digests[:n]) or \
            any(len(d) != 32 for p in received_column_paths for d in p):
        raise _verifier_error("ColumnEval", "digest is not 32 bytes")
    leaves = np.frombuffer(b"".join(received_columns_digests[:n]), np.uint8).copy()
    paths = np.frombuffer(b"".join(b"".join(p) for p in received_column_paths) or b"\0", np.uint8).copy()
    idx = np.ascontiguousarray(np.array(requested_columns, dtype=np.uint64))
    ok = np.zeros(n, np.uint8)
    rp, keep = _u8p(root)
    _raise(N.load().lcpc_verify_leaf_paths(leaves.ctypes.data_as(N.u8p), paths.ctypes.data_as(N.u8p), n, plen,
                                           _p64(idx), rp, ok.ctypes.data_as(N.u8p)))
    if not ok.all():
        raise _verifier_error("ColumnEval", "Merkle path mismatch")


def hash_field_vec_to_digest(column, field: int = FT63) -> bytes:
    """lcpc_online.rs:439-452: BLAKE3(32 zero bytes || repr of every element)."""
    return hash_columns_to_digests([column], field)[0]


def hash_column_to_digest(column: LcColumn, field: int = FT63) -> bytes:
    """lcpc_online.rs:431-437."""
    return hash_field_vec_to_digest(column.col, field)


def hash_columns_to_digests(columns, field: int = FT63) -> List[bytes]:
    """hash_column_to_digest over many columns in one GPU launch."""
    cols = [np.ascontiguousarray(getattr(c, "col", c), dtype=np.uint64).reshape(-1) for c in columns]
    if not cols:
        return []
    n_rows = cols[0].size // limbs(field)
    if any(c.size != cols[0].size for c in cols):
        raise ValueError("columns of different lengths")
    m = np.ascontiguousarray(np.concatenate(cols)) if n_rows else np.zeros(1, np.uint64)
    out = np.zeros(32 * len(cols), np.uint8)
    _raise(N.load().lcpc_hash_field_columns(field, _p64(m), n_rows, len(cols), out.ctypes.data_as(N.u8p)))
    return [out[32 * i:32 * i + 32].tobytes() for i in range(len(cols))]


def client_online_verify_column_leaves(locally_derived_column_leaves: Sequence[bytes],
                                       requested_columns: Sequence[int],
                                       received_column_leaves: Sequence[bytes]) -> None:
    """lcpc_online.rs:321-356 (errors are NumColOpens there, kept)."""
    if (len(locally_derived_column_leaves) != len(requested_columns)
            or len(received_column_leaves) != len(requested_columns)):
        raise _verifier_error("NumColOpens", "leaf count")
    if any(bytes(a) != bytes(b) for a, b in zip(locally_derived_column_leaves, received_column_leaves)):
        raise _verifier_error("NumColOpens", "leaf mismatch")


def _get_POS_soundness_n_cols(pre_encoded_columns: int, encoded_columns: int) -> int:  # noqa: N802
    """lcpc_online.rs:363-368 (f64 arithmetic as in Rust)."""
    den = math.log2((1.0 + pre_encoded_columns / encoded_columns) / 2.0)
    return min(math.ceil(-128.0 / den), encoded_columns)


def get_PoS_soudness_n_cols(num_columns: int, num_encoded_columns: int) -> int:  # noqa: N802
    """lcpc_online.rs:359-361 (FileMetadata's two widths passed directly)."""
    return _get_POS_soundness_n_cols(num_columns, num_encoded_columns)


def client_verify_commitment(root: bytes, locally_derived_column_leaves: Sequence[bytes],
                             requested_columns: Sequence[int], received_columns: Sequence[LcColumn],
                             required_columns_for_soundness: int, field: int = FT63) -> None:
    """lcpc_online.rs:370-398: the received columns hash to the locally derived leaves and their
    paths lead to root."""
    if (required_columns_for_soundness < len(locally_derived_column_leaves)
            or required_columns_for_soundness < len(requested_columns)
            or required_columns_for_soundness < len(received_columns)):
        raise _verifier_error("NumColOpens", "more columns than the soundness count")
    received_leaves = hash_columns_to_digests(received_columns, field)
    client_online_verify_column_leaves(locally_derived_column_leaves, requested_columns, received_leaves)
    client_online_verify_column_paths(root, requested_columns, received_columns, field)


def client_verify_commitment_without_full_columns(root: bytes, locally_derived_column_leaves: Sequence[bytes],
                                                  requested_columns: Sequence[int],
                                                  received_column_digests: Sequence[bytes],
                                                  received_column_paths: Sequence[Sequence[bytes]],
                                                  required_columns_for_soundness: int) -> None:
    """lcpc_online.rs:400-429."""
    if (required_columns_for_soundness < len(locally_derived_column_leaves)
            or required_columns_for_soundness < len(requested_columns)
            or required_columns_for_soundness < len(received_column_digests)):
        raise _verifier_error("NumColOpens", "more columns than the soundness count")
    client_online_verify_column_leaves(locally_derived_column_leaves, requested_columns, received_column_digests)
    client_online_verify_column_paths_without_full_columns(root, requested_columns, received_column_digests,
                                                           received_column_paths)


def verify_proper_partial_polynomial_evaluation(left_evaluation_column, evaluation_result_vector,
                                                requested_columns_indices: Sequence[int],
                                                received_columns: Sequence[LcColumn],
                                                field: int = FT63) -> None:
    """lcpc_online.rs:487-516: vector_multiply(left, column) == the result entry of that column.
    As in the reference, the result entries are taken in increasing column index (the filter
    over the result vector) and zipped with the columns in the order received."""
    nl = limbs(field)
    res = np.ascontiguousarray(np.asarray(evaluation_result_vector, dtype=np.uint64).reshape(-1))
    n_res = res.size // nl
    wanted = set(int(i) for i in requested_columns_indices)
    picked = [i for i in range(n_res) if i in wanted]
    k = min(len(received_columns), len(picked))
    if k == 0:
        return
    cols = np.ascontiguousarray(np.concatenate(
        [np.asarray(getattr(c, "col", c), dtype=np.uint64).reshape(-1) for c in received_columns[:k]]))
    n_rows = cols.size // nl // k
    left = np.ascontiguousarray(np.asarray(left_evaluation_column, dtype=np.uint64).reshape(-1))
    if left.size // nl < n_rows:
        raise _verifier_error("ColumnEval", "left vector shorter than the columns")
    idx = np.array(picked[:k], dtype=np.uint64)
    ok = np.zeros(k, np.uint8)
    _raise(N.load().lcpc_verify_column_values(field, _p64(cols), k, n_rows, _p64(left), _p64(res), n_res,
                                              _p64(idx), ok.ctypes.data_as(N.u8p)))
    if not ok.all():
        raise _verifier_error("ColumnEval", "column value mismatch")


def verifiable_full_polynomial_evaluation(left_evaluation_column, right_evaluation_column,
                                          received_decoded_result_vector, requested_column_indices,
                                          received_columns, pre_encoded_len: int, encoded_len: int,
                                          field: int = FT63):
    """lcpc_online.rs:519-543.  The reference body does not compile as written (it passes an
    undefined `received_result_vector`); this restates its evident intent: the result is
    <decoded u^T M, right>, and the decoded vector re-encoded (Enc(u^T M) = u^T Enc(M)) must
    agree with u^T col at every opened column.  Parity unpinned (no reference output exists)."""
    nl = limbs(field)
    dec = np.ascontiguousarray(np.asarray(received_decoded_result_vector, dtype=np.uint64).reshape(-1, nl))
    right = np.ascontiguousarray(np.asarray(right_evaluation_column, dtype=np.uint64).reshape(-1, nl))
    result = field_dot(dec[:pre_encoded_len], right[:pre_encoded_len], field)
    enc = LigeroEncoding.new_from_dims(field, pre_encoded_len, encoded_len)
    row = np.zeros((encoded_len, nl), np.uint64)
    row[:min(pre_encoded_len, dec.shape[0])] = dec[:pre_encoded_len]
    encoded = enc.encode(row)
    verify_proper_partial_polynomial_evaluation(left_evaluation_column, encoded, requested_column_indices,
                                                received_columns, field)
    return result


def verify_full_polynomial_evaluation_wrapper_with_single_eval_point(
        evaluation_point, received_result_vector, n_rows: int, n_cols: int, requested_column_indices,
        received_columns, pre_encoded_len: int, field: int = FT63):
    """lcpc_online.rs:545-566 (side vectors from the point, then the check above)."""
    left, right = form_side_vectors_for_polynomial_evaluation_from_point(evaluation_point, n_rows, n_cols, field)
    return verifiable_full_polynomial_evaluation(left, right, received_result_vector, requested_column_indices,
                                                 received_columns, pre_encoded_len, n_cols, field)


def left_multiply_unencoded_matrix_by_vector(data: bytes, pre_encoded_size: int, left_vector) -> np.ndarray:
    """file_handler.rs:614-638: u^T M over the file's unencoded rows (7 bytes per element, rows of
    pre_encoded_size), read straight from the bytes (lcpc_pos_left_multiply_bytes).  The reference
    returns an empty vector (its result is `with_capacity` and never resized); this
    returns the sum it is written to accumulate."""
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    n_rows = -(-(-(-a.size // DATA_BYTE_CAPACITY)) // pre_encoded_size)
    left = np.ascontiguousarray(np.asarray(left_vector, dtype=np.uint64).reshape(-1))
    if left.size != n_rows:
        raise ValueError(f"left_vector incorrect size, expected {n_rows} and received {left.size}")
    out = np.zeros((pre_encoded_size, 1), np.uint64)
    _raise(N.load().lcpc_pos_left_multiply_bytes(a.ctypes.data, a.size, pre_encoded_size, _p64(left), left.size,
                                                 _p64(out)))
    return out


# ---------------------------------------------------------------- update audits
# The evaluation request after an edit, an append or a reshape (messages: networking/shared.rs:90-129,
# 165-188; server: networking/server.rs:833-906, 963-1077; client: networking/client.rs:755-827,
# 1009-1135, 1273-1420).  Restated where the reference is inconsistent: the rows an
# update touches follow the single rule of lcpc_pos_update_rows, the client checks the opened
# columns against both roots and the touched rows against its own bytes, and a no-op edit passes.
FT63_MODULUS = 5102708120182849537  # lcpc-test-fields/src/lib.rs:18-22
EVAL_POLY_TILE = 2048               # coefficients per block of the evaluation kernel (pos.hpp)
EVAL_STAGE_BYTES = 7 << 20          # LCPC_POS_EVAL_STAGE_BYTES


@dataclass
class ReshapeEvaluation:
    """ServerMessages::ReshapeEvaluation (shared.rs:165-171)."""
    expected_result: np.ndarray
    original_result_vector: np.ndarray
    original_columns: List[LcColumn]
    new_result_vector: np.ndarray
    new_columns: List[LcColumn]
    original_root: bytes = b""   # not part of the message: the roots the server computed
    new_root: bytes = b""


@dataclass
class UpdateEvaluation:
    """ServerMessages::EditEvaluation / AppendEvaluation (shared.rs:172-188) as one message:
    original_bytes = the old file's bytes of the touched rows (lcpc_pos_update_rows)."""
    original_result_vector: np.ndarray
    original_columns: List[LcColumn]
    new_result_vector: np.ndarray
    new_columns: List[LcColumn]
    original_bytes: bytes
    original_root: bytes = b""   # not part of the message: the roots the server computed
    new_root: bytes = b""


def update_rows(old_len: int, offset: int, length: int, pre: int) -> tuple:
    """lcpc_pos_update_rows: (row_lo, row_hi, old_lo, old_hi) of writing `length` bytes at `offset`
    into a file of old_len bytes.  Host only."""
    r = [C.c_size_t() for _ in range(4)]
    _raise(N.load().lcpc_pos_update_rows(old_len, offset, length, pre, *[C.byref(v) for v in r]))
    return tuple(v.value for v in r)


class _DeviceImage:
    """A file image in device memory for one server call, through the HIP runtime the library links."""

    def __init__(self, data):
        N.load()
        self._rt = C.CDLL("libamdhip64.so.7")
        self._rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self._rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self._rt.hipFree.argtypes = [C.c_void_p]
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(data, np.uint8)
        self.n = a.size
        p = C.c_void_p()
        if self._rt.hipMalloc(C.byref(p), self.n + 16) != 0:
            _raise(32)
        self.ptr = p.value
        if self.n and self._rt.hipMemcpy(self.ptr, a.ctypes.data, self.n, 1) != 0:
            self._rt.hipFree(self.ptr)
            _raise(31)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._rt.hipFree(self.ptr)


def _columns(cols: np.ndarray, paths, n: int, path_len: int) -> List[LcColumn]:
    pb = bytes(paths)
    return [LcColumn(cols[k].copy(), [pb[32 * (k * path_len + i):32 * (k * path_len + i + 1)] for i in range(path_len)])
            for k in range(n)]


def _update_evaluation(enc_old: LigeroEncoding, d_old: int, n_old: int, enc_new: LigeroEncoding, d_new: int,
                       n_new: int, point, cols_old, cols_new, want_expected: bool):
    """lcpc_pos_update_evaluation: ((result, columns, root) old, the same new, expected or None)."""
    x = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1)[:1].copy()
    sides = []
    for enc, n, cols in ((enc_old, n_old, cols_old), (enc_new, n_new, cols_new)):
        idx = np.ascontiguousarray(list(cols), dtype=np.uint64)
        n_rows = -(-(-(-n // DATA_BYTE_CAPACITY)) // enc.n_per_row)
        pl = (enc.n_cols - 1).bit_length()
        sides.append(dict(idx=idx, pl=pl, result=np.zeros((enc.n_cols, 1), np.uint64),
                          cols=np.zeros((max(idx.size, 1), n_rows, 1), np.uint64),
                          paths=(C.c_uint8 * max(32 * pl * idx.size, 1))(), root=(C.c_uint8 * 32)()))
    expected = np.zeros((1, 1), np.uint64)
    args = [enc_old._h, d_old, n_old, enc_new._h, d_new, n_new, _p64(x)]
    for s in sides:
        args += [_p64(s["idx"]) if s["idx"].size else None, s["idx"].size]
    for s in sides:
        args += [_p64(s["result"]), _p64(s["cols"]), C.cast(s["paths"], N.u8p), C.cast(s["root"], N.u8p)]
    _raise(N.load().lcpc_pos_update_evaluation(*args, _p64(expected) if want_expected else None))
    out = [(s["result"], _columns(s["cols"], s["paths"], s["idx"].size, s["pl"]), bytes(s["root"])) for s in sides]
    return out[0], out[1], (expected if want_expected else None)


def server_reshape_evaluation(data, old_dims, new_dims, point, cols_old, cols_new) -> ReshapeEvaluation:
    """The reshape handler (server.rs:833-906): the one file committed under both shapes, the columns
    of each opened, and the file polynomial's value at the point.  dims = (pre, enc)."""
    enc_old = LigeroEncoding.new_from_dims(FT63, *old_dims)
    enc_new = LigeroEncoding.new_from_dims(FT63, *new_dims)
    with _DeviceImage(data) as d:
        old, new, expected = _update_evaluation(enc_old, d.ptr, d.n, enc_new, d.ptr, d.n, point, cols_old, cols_new,
                                                True)
    return ReshapeEvaluation(expected, old[0], old[1], new[0], new[1], old[2], new[2])


def server_update_evaluation(old_data, new_data, dims, point, cols, offset: Optional[int] = None,
                             length: Optional[int] = None) -> UpdateEvaluation:
    """The edit and append handler (server.rs:963-1077): both versions committed under dims = (pre,
    enc), the same columns of each opened, and the old file's bytes of the rows the update touched.
    offset / length: the update's byte range as the client sent it; left out, the range from the first
    to the last byte in which the versions differ (an append: from the old end)."""
    old_data, new_data = bytes(old_data), bytes(new_data)
    if offset is None or length is None:
        m = min(len(old_data), len(new_data))
        ne = np.flatnonzero(np.frombuffer(old_data[:m], np.uint8) != np.frombuffer(new_data[:m], np.uint8))
        lo = int(ne[0]) if ne.size else len(old_data)
        hi = len(new_data) if len(new_data) > len(old_data) else (int(ne[-1]) + 1 if ne.size else 0)
        if len(new_data) < len(old_data) or hi <= lo:
            raise ValueError("the versions are equal (or the file shrank): give the update's offset and length")
        offset, length = lo, hi - lo
    _, _, old_lo, old_hi = update_rows(len(old_data), offset, length, dims[0])
    enc = LigeroEncoding.new_from_dims(FT63, *dims)
    with _DeviceImage(old_data) as d_old, _DeviceImage(new_data) as d_new:
        old, new, _ = _update_evaluation(enc, d_old.ptr, d_old.n, enc, d_new.ptr, d_new.n, point, cols, cols, False)
    return UpdateEvaluation(old[0], old[1], new[0], new[1], old_data[old_lo:old_hi], old[2], new[2])


def _file_rows(n_bytes: int, pre: int) -> int:
    return -(-(-(-n_bytes // DATA_BYTE_CAPACITY)) // pre)


def client_verify_evaluation(root: bytes, n_bytes: int, pre: int, enc: int, point, cols, result_vector,
                             columns: Sequence[LcColumn]) -> np.ndarray:
    """The client's check of one plain audit response (FileHandler.polynomial_evaluation_response):
    the opened columns hash up to root, and the decoded result vector, re-encoded, agrees with them
    (checks 1 and 2 of the update audits, for one version); returns the file polynomial's value at
    the point.  Raises VerifierError (ColumnEval); non-increasing columns raise ValueError.  Many
    responses at once: client_verify_evaluations_grouped."""
    cols = [int(c) for c in cols]
    if any(b <= a for a, b in zip(cols, cols[1:])):
        raise ValueError("requested columns must be strictly increasing")
    n_rows = _file_rows(n_bytes, pre)
    if len(columns) != len(cols) or any(np.asarray(c.col).size != n_rows for c in columns):
        raise _verifier_error("ColumnEval", "opened columns do not have the file's row count")
    res = np.ascontiguousarray(np.asarray(result_vector, dtype=np.uint64).reshape(-1, 1))
    if res.shape[0] != enc:
        raise _verifier_error("ColumnEval", "result vector is not one encoded row")
    client_online_verify_column_paths(root, cols, columns)
    # side vectors over (n_rows, pre): the left stride is pre, so the value is the file polynomial's
    left, right = form_side_vectors_for_polynomial_evaluation_from_point(point, n_rows, pre)
    return verifiable_full_polynomial_evaluation(left, right, decode_row(res), cols, columns, pre, enc)


_checked_file_evaluation = client_verify_evaluation   # the name the update audits know it by


def client_verify_reshape_evaluation(old_root: bytes, new_root: bytes, file_len: int, old_dims, new_dims, point,
                                     cols_old, cols_new, response: ReshapeEvaluation) -> np.ndarray:
    """client.rs:755-827: both shapes' evaluations verify against their roots and agree with each
    other and with expected_result.  Returns the evaluation; raises VerifierError (ColumnEval,
    ReshapeMismatch)."""
    old = _checked_file_evaluation(old_root, file_len, old_dims[0], old_dims[1], point, cols_old,
                                   response.original_result_vector, response.original_columns)
    new = _checked_file_evaluation(new_root, file_len, new_dims[0], new_dims[1], point, cols_new,
                                   response.new_result_vector, response.new_columns)
    want = np.asarray(response.expected_result, dtype=np.uint64).reshape(-1)
    if not (np.array_equal(old.reshape(-1), new.reshape(-1)) and np.array_equal(new.reshape(-1), want)):
        raise _verifier_error("ReshapeMismatch", "the two shapes do not evaluate to the expected result")
    return new


def client_verify_update_evaluation(old_root: bytes, new_root: bytes, old_len: int, offset: int, data: bytes,
                                    pre: int, enc: int, point, cols, response: UpdateEvaluation) -> np.ndarray:
    """client.rs:1009-1135, 1273-1420: the client wrote `data` at `offset` into its file of old_len
    bytes (kept as old_root) and was given new_root.  Accepts new_root only if (1) the opened columns
    hash up to the two roots, (2) both result vectors agree with them, (4) the touched rows of both
    versions, encoded here from original_bytes and the client's own data, are what the columns hold
    and every other row is unchanged, and (5) the evaluations differ by what those rows predict.
    Returns the new evaluation; raises VerifierError (ColumnEval, RowsMismatch, UpdateMismatch)."""
    data = bytes(data)
    row_lo, row_hi, old_lo, old_hi = update_rows(old_len, offset, len(data), pre)
    new_len = max(old_len, offset + len(data))
    cols = [int(c) for c in cols]
    old_val = _checked_file_evaluation(old_root, old_len, pre, enc, point, cols, response.original_result_vector,
                                       response.original_columns)
    new_val = _checked_file_evaluation(new_root, new_len, pre, enc, point, cols, response.new_result_vector,
                                       response.new_columns)
    # (4) the rows are authentic (a TODO in the reference, client.rs:1325-1327)
    old_rows = bytes(response.original_bytes)
    if len(old_rows) != old_hi - old_lo:
        raise _verifier_error("RowsMismatch", "original_bytes is not the touched rows' length")
    rel = offset - old_lo
    spliced = bytearray(old_rows) + bytes(max(0, rel + len(data) - len(old_rows)))
    spliced[rel:rel + len(data)] = data
    new_rows = bytes(spliced)
    rb = pre * DATA_BYTE_CAPACITY
    n_rows_old, n_rows_new = _file_rows(old_len, pre), _file_rows(new_len, pre)
    code = LigeroEncoding.new_from_dims(FT63, pre, enc)
    for rows, n_rows, columns in ((old_rows, n_rows_old, response.original_columns),
                                  (new_rows, n_rows_new, response.new_columns)):
        n = -(-len(rows) // rb)
        if n == 0 or not cols:
            continue
        m = np.zeros((n, enc, 1), np.uint64)
        for i in range(n):
            el = convert_byte_vec_to_field_elements_vec(rows[i * rb:(i + 1) * rb])
            m[i, :el.shape[0]] = el
        m = code.encode_rows(m)
        for k, c in enumerate(cols):
            col = np.asarray(columns[k].col, dtype=np.uint64).reshape(-1)
            if not np.array_equal(m[:, c, 0], col[row_lo:row_lo + n]):
                raise _verifier_error("RowsMismatch", "an opened column disagrees with the touched rows")
    for k in range(len(cols)):
        a = np.asarray(response.original_columns[k].col, dtype=np.uint64).reshape(-1)
        b = np.asarray(response.new_columns[k].col, dtype=np.uint64).reshape(-1)
        keep = np.ones(n_rows_old, bool)
        keep[row_lo:row_hi] = False
        if not np.array_equal(a[:n_rows_old][keep], b[:n_rows_old][keep]):
            raise _verifier_error("RowsMismatch", "an untouched row changed")
    # (5) the difference of the evaluations is the difference of the touched rows' polynomials
    d = row_lo * pre
    p_old = evaluate_bytes_polynomial_at_point(old_rows, point, d) if old_rows else np.zeros((1, 1), np.uint64)
    p_new = evaluate_bytes_polynomial_at_point(new_rows, point, d)
    lhs = (int(new_val.reshape(-1)[0]) - int(old_val.reshape(-1)[0])) % FT63_MODULUS
    rhs = (int(p_new.reshape(-1)[0]) - int(p_old.reshape(-1)[0])) % FT63_MODULUS
    if lhs != rhs:
        raise _verifier_error("UpdateMismatch", "the evaluations do not differ by the update's polynomial")
    return new_val


def client_verify_edit_evaluation(old_root: bytes, new_root: bytes, file_len: int, offset: int, data: bytes,
                                  pre: int, enc: int, point, cols, response: UpdateEvaluation) -> np.ndarray:
    """The edit flow (client.rs:1273-1420): an update inside the file."""
    if offset + len(data) > file_len:
        raise ValueError("an edit stays inside the file")
    return client_verify_update_evaluation(old_root, new_root, file_len, offset, data, pre, enc, point, cols, response)


def client_verify_append_evaluation(old_root: bytes, new_root: bytes, old_len: int, data: bytes, pre: int, enc: int,
                                    point, cols, response: UpdateEvaluation) -> np.ndarray:
    """The append flow (client.rs:1009-1135): an update at the old end."""
    return client_verify_update_evaluation(old_root, new_root, old_len, old_len, data, pre, enc, point, cols, response)


# ---------------------------------------------------------------- checkable reads
# Reading a byte range so that the client can check it against its root (include/lcpc_mi.h, "PoS
# checkable reads").  No counterpart in the reference: RequestFileRow (networking/
# server.rs:474-493) answers with bytes the client has to trust.
#
# THE ORDER OF THE TWO MESSAGES IS A SOUNDNESS CONDITION.  The client first receives the rows
# (FileHandler.read_rows_response) and only then draws the columns and asks for the openings
# (FileHandler.read_opening_response).  A server that knows the columns before it sends the rows
# can interpolate a wrong row that agrees with the committed one at every one of them.
READ_COVER_CAP = 128   # cover nodes of any size_t chunk count


@dataclass
class ReadPlan:
    """lcpc_pos_read_plan: the rows [row_lo, row_hi) that hold the byte range, the 1-KiB leaf chunks
    [chunk_lo, chunk_hi) that hold those rows, the rows [seg_row_lo, seg_row_hi) of those chunks, and
    the cover nodes (chunk lo, chunk hi) in walk order."""
    row_lo: int
    row_hi: int
    chunk_lo: int
    chunk_hi: int
    seg_row_lo: int
    seg_row_hi: int
    cover_nodes: List[tuple]

    @property
    def n_cover(self) -> int:
        return len(self.cover_nodes)


@dataclass
class ReadOpening:
    """The server's second message: per requested column its segment (rows [seg_row_lo, seg_row_hi)
    as canonical 8-byte values, the `.porenc`'s own bytes), its cover values and its Merkle path."""
    segments: np.ndarray          # (n_columns, seg_rows) uint64, canonical
    covers: np.ndarray            # (n_columns, n_cover, 32) uint8
    paths: List[List[bytes]]      # per column log2(enc) digests

    def n_bytes(self) -> int:
        return int(np.asarray(self.segments).size * 8 + np.asarray(self.covers).size
                   + sum(len(d) for p in self.paths for d in p))


def read_plan(file_len: int, byte_start: int, byte_end: int, pre: int) -> ReadPlan:
    """lcpc_pos_read_plan.  Host only."""
    r = [C.c_size_t() for _ in range(7)]
    nodes = (C.c_size_t * (2 * READ_COVER_CAP))()
    _raise(N.load().lcpc_pos_read_plan(file_len, byte_start, byte_end, pre, *[C.byref(v) for v in r], nodes,
                                       READ_COVER_CAP))
    v = [x.value for x in r]
    return ReadPlan(*v[:6], [(nodes[2 * j], nodes[2 * j + 1]) for j in range(v[6])])


def _n_covers(rows_written: int, chunk_lo: int, chunk_hi: int) -> int:
    """The cover count of a chunk range: the plan of a byte range that selects exactly those chunks."""
    n_chunks = N.load().lcpc_leaf_n_chunks(FT63, rows_written)
    first = N.load().lcpc_leaf_chunk_first_row(FT63, chunk_lo)
    last = (rows_written if chunk_hi >= n_chunks else N.load().lcpc_leaf_chunk_first_row(FT63, chunk_hi)) - 1
    return read_plan(7 * rows_written, 7 * first, 7 * last + 1, 1).n_cover


def segment_covers_from_cache(cache, columns, chunk_lo: int, chunk_hi: int) -> np.ndarray:
    """lcpc_pos_segment_covers_from_cache: (n_columns, n_cover, 32) cover values of the columns opened
    on chunks [chunk_lo, chunk_hi), from a pos_files.ColumnChunkCache (left untouched)."""
    idx = np.ascontiguousarray(list(columns), dtype=np.uint64)
    out = np.zeros((idx.size, _n_covers(cache.rows, chunk_lo, chunk_hi), 32), np.uint8)
    _raise(N.load().lcpc_pos_segment_covers_from_cache(cache._h, _p64(idx) if idx.size else None, idx.size,
                                                       chunk_lo, chunk_hi, out.ctypes.data_as(N.u8p)))
    return out


def segment_covers_from_columns(cols, rows_written: int, chunk_lo: int, chunk_hi: int) -> np.ndarray:
    """lcpc_pos_segment_covers_from_columns: the same bytes from the whole opened columns
    ((n_columns, rows_written) canonical values) when the server keeps no cache."""
    a = np.ascontiguousarray(cols, dtype=np.uint64).reshape(-1, rows_written)
    out = np.zeros((a.shape[0], _n_covers(rows_written, chunk_lo, chunk_hi), 32), np.uint8)
    _raise(N.load().lcpc_pos_segment_covers_from_columns(_p64(a), rows_written, a.shape[0], chunk_lo, chunk_hi,
                                                         out.ctypes.data_as(N.u8p)))
    return out


def segment_leaves(segments, rows_written: int, chunk_lo: int, chunk_hi: int, covers, weights=None):
    """lcpc_pos_segment_leaves: (leaves (n, 32) uint8, dots (n,) Montgomery limbs or None,
    canonical_ok (n,) bool) for n segments (n, seg_rows) and their covers (n, n_cover, 32)."""
    seg = np.ascontiguousarray(segments, dtype=np.uint64)
    n = seg.shape[0]
    seg = seg.reshape(n, -1)
    cov = np.ascontiguousarray(covers, dtype=np.uint8).reshape(n, -1, 32)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1)
    if w is not None and w.size != seg.shape[1]:
        raise ValueError("one weight per segment row")
    leaves = np.zeros((n, 32), np.uint8)
    dots = None if w is None else np.zeros(n, np.uint64)
    ok = np.zeros(n, np.uint8)
    _raise(N.load().lcpc_pos_segment_leaves(
        _p64(seg) if seg.size else None, n, rows_written, chunk_lo, chunk_hi,
        cov.ctypes.data_as(N.u8p) if cov.size else None, cov.shape[1],
        None if w is None else _p64(w), leaves.ctypes.data_as(N.u8p), None if dots is None else _p64(dots),
        ok.ctypes.data_as(N.u8p)))
    return leaves, dots, ok.astype(bool)


def _verify_read(code: LigeroEncoding, root: bytes, file_len: int, byte_start: int, byte_end: int, data: bytes,
                 columns, opening: ReadOpening, seed: Optional[int] = None) -> bytes:
    """client_verify_read under a given encoding (its dims are the file's)."""
    if code.digest != 0:
        raise DeviceError(34, "a checkable read is BLAKE3-only; the encoding's digest is "
                          f"{digest_name(code.digest)}")   # LCPC_ERR_UNSUPPORTED, as the other stored-file entries
    pre, enc = code.n_per_row, code.n_cols
    plan = read_plan(file_len, byte_start, byte_end, pre)
    cols = [int(c) for c in columns]
    if any(b <= a for a, b in zip(cols, cols[1:])) or any(not 0 <= c < enc for c in cols):
        raise ValueError("requested columns must be strictly increasing and below enc")
    rb = pre * DATA_BYTE_CAPACITY
    rows_written = _file_rows(file_len, pre)
    data = bytes(data)
    lo_byte = plan.row_lo * rb
    if len(data) != min(plan.row_hi * rb, file_len) - lo_byte:
        raise _verifier_error("ColumnEval", "data is not the whole rows that cover the range")
    n, seg_rows = len(cols), plan.seg_row_hi - plan.seg_row_lo
    seg = np.asarray(opening.segments)
    cov = np.asarray(opening.covers)
    if seg.dtype != np.uint64 or seg.shape != (n, seg_rows):
        raise _verifier_error("ColumnEval", "segments are not one per column of the chunk range's rows")
    if cov.dtype != np.uint8 or cov.shape != (n, plan.n_cover, 32):
        raise _verifier_error("ColumnEval", "cover count")
    if len(opening.paths) != n:
        raise _verifier_error("ColumnEval", "path count")
    if n == 0:
        return data[byte_start - lo_byte:byte_end - lo_byte]
    # a private u over the rows read; the segment's other rows are only hashed (weight zero)
    n_rows = plan.row_hi - plan.row_lo
    if seed is None:
        import secrets
        u = np.array([secrets.randbelow(FT63_MODULUS) for _ in range(n_rows)], np.uint64)
    else:
        u = np.random.default_rng(seed).integers(0, FT63_MODULUS, n_rows, dtype=np.uint64)
    weights = np.zeros(seg_rows, np.uint64)
    weights[plan.row_lo - plan.seg_row_lo:plan.row_hi - plan.seg_row_lo] = u
    # (1) canonical elements and (2) the rebuilt leaves reach the root
    leaves, dots, ok = segment_leaves(seg, rows_written, plan.chunk_lo, plan.chunk_hi, cov, weights)
    if not ok.all():
        raise _verifier_error("ColumnEval", "a segment element is not canonical")
    client_online_verify_column_paths_without_full_columns(root, cols, [leaves[k].tobytes() for k in range(n)],
                                                           opening.paths)
    # (3) Enc(u^T M) over the received bytes agrees with u^T segment at every opened column
    row = np.zeros((enc, 1), np.uint64)
    row[:pre] = left_multiply_unencoded_matrix_by_vector(data, pre, u)
    encoded = code.encode(row).reshape(-1)
    if not np.array_equal(encoded[np.array(cols, dtype=np.int64)], dots):
        raise _verifier_error("ReadMismatch", "the rows received are not the rows the opened columns commit to")
    return data[byte_start - lo_byte:byte_end - lo_byte]


def client_verify_read(root: bytes, file_len: int, pre: int, enc: int, byte_start: int, byte_end: int, data: bytes,
                       columns, opening: ReadOpening, seed: Optional[int] = None) -> bytes:
    """Accepts bytes [byte_start, byte_end) of the file committed as root (file_len bytes, dims pre /
    enc) and returns exactly them, or raises.  data: the server's first message, the whole rows that
    cover the range; columns: the indices the client drew AFTER it held data (strictly increasing,
    below enc; get_PoS_soudness_n_cols(pre, enc) of them for the full soundness) -- a server that
    learns them before it sends data can forge a row that passes; opening: its second message.

    Checks: every segment element is canonical; each leaf rebuilt from segment and covers hashes up
    its path to root; and with a private random u over the rows read (secrets; `seed` only for tests),
    Enc(u^T data)[j] = sum_r u_r segment_j[r] at every opened column j.  Wrong lengths, a wrong cover
    count, a non-canonical element or a leaf that does not reach root raise VerifierError(ColumnEval);
    rows that disagree with the openings raise VerifierError(ReadMismatch)."""
    return _verify_read(LigeroEncoding.new_from_dims(FT63, pre, enc), root, file_len, byte_start, byte_end, data,
                        columns, opening, seed)


# ---------------------------------------------------------------- batched audits of a stored file
# m evaluation points, one pass over the raw file, one set of opened columns.  No
# counterpart in the reference, whose server answers one point per request.
LEFT_MANY_PACK, LEFT_MANY_VALU, LEFT_MANY_MFMA = 0, 1, 2


def left_multiply_many_kernel(pre_encoded_size: int, n_vecs: int) -> int:
    """The kernel left_multiply_unencoded_matrix_by_vectors runs for this shape: LEFT_MANY_PACK (the
    image is packed to elements first), LEFT_MANY_VALU or LEFT_MANY_MFMA (the int8 matrix cores).
    A pure function of its arguments and LCPC_NO_MFMA; needs no device."""
    return int(N.load().lcpc_pos_left_multiply_many_kernel(pre_encoded_size, n_vecs))


def left_multiply_unencoded_matrix_by_vectors(data, pre_encoded_size: int, lefts) -> np.ndarray:
    """left_multiply_unencoded_matrix_by_vector for m left vectors in one pass over the bytes
    (lcpc_pos_left_multiply_bytes_many): lefts is (m, n_rows) Montgomery words, the result (m,
    pre_encoded_size), row j bit for bit the single call's vector for lefts[j]."""
    a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8)
    n_rows = _file_rows(a.size, pre_encoded_size)
    lv = np.ascontiguousarray(np.asarray(lefts, dtype=np.uint64))
    lv = lv.reshape(lv.shape[0], -1) if lv.ndim > 1 else lv.reshape(1, -1)
    if lv.shape[1] != n_rows:
        raise ValueError(f"left vectors of incorrect size, expected {n_rows} and received {lv.shape[1]}")
    out = np.zeros((lv.shape[0], pre_encoded_size), np.uint64)
    _raise(N.load().lcpc_pos_left_multiply_bytes_many(a.ctypes.data, a.size, pre_encoded_size, _p64(lv.reshape(-1)),
                                                      lv.shape[0], n_rows, _p64(out.reshape(-1))))
    return out


# ---------------------------------------------------------------- grouped audits of many stored files
# A server's queue of audits over different files, most of them small, answered with launches that
# do not grow with the number of files.  No counterpart in the reference.
GROUP_STAGE_BYTES = 32 << 20        # LCPC_POS_GROUP_STAGE_BYTES
GROUP_SINGLE = 0xFFFFFFFF           # LCPC_POS_GROUP_SINGLE: a job routed to the single-file path


def _as_image(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, np.uint8)
    return np.ascontiguousarray(np.asarray(data, np.uint8).reshape(-1))


def _sizes(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(values), dtype=np.uint64)).astype(C.c_size_t)


def _group_lefts(sizes, pres, lefts):
    """the jobs' left vectors one after another, checked against the files' row counts"""
    flat = []
    for j, (n, pre, lv) in enumerate(zip(sizes, pres, lefts)):
        v = np.asarray(lv, dtype=np.uint64).reshape(-1)
        if v.size != _file_rows(int(n), int(pre)):
            raise ValueError(f"job {j}: left_vector incorrect size, expected {_file_rows(int(n), int(pre))} "
                             f"and received {v.size}")
        flat.append(v)
    return np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros(0, np.uint64)


def _split_outputs(out: np.ndarray, pres) -> List[np.ndarray]:
    ends = np.cumsum(np.asarray(pres, dtype=np.int64))
    return [out[e - int(p):e].reshape(-1, 1) for e, p in zip(ends, pres)]


def left_multiply_unencoded_matrices_by_vectors(datas, pres, lefts) -> List[np.ndarray]:
    """left_multiply_unencoded_matrix_by_vector for many files in one call
    (lcpc_pos_left_multiply_bytes_grouped): job j is the file datas[j] with rows of pres[j] elements
    and the left vector lefts[j].  Returns the list of (pres[j], 1) arrays, array j word for word what
    left_multiply_unencoded_matrix_by_vector(datas[j], pres[j], lefts[j]) returns; the launches are
    per staging group of files, not per file."""
    images = [_as_image(d) for d in datas]
    pres = [int(p) for p in pres]
    if not (len(images) == len(pres) == len(lefts)):
        raise ValueError("datas, pres and lefts must have one entry per job")
    if not images:
        return []
    if any(a.size == 0 for a in images) or any(p < 1 for p in pres):
        raise ValueError("every job needs a non-empty file and pre_encoded_size >= 1")
    sizes = [a.size for a in images]
    lv = _group_lefts(sizes, pres, lefts)
    out = np.zeros(sum(pres), np.uint64)
    ptrs = (C.c_void_p * len(images))(*[a.ctypes.data for a in images])
    nb, pr = _sizes(sizes), _sizes(pres)
    _raise(N.load().lcpc_pos_left_multiply_bytes_grouped(ptrs, nb.ctypes.data_as(N.szp), pr.ctypes.data_as(N.szp),
                                                         len(images), _p64(lv), lv.size, _p64(out), out.size))
    return _split_outputs(out, pres)


def left_multiply_device_arena_by_vectors(arena_ptr: int, offsets, sizes, pres, lefts) -> List[np.ndarray]:
    """The same over a device arena the caller owns (lcpc_pos_left_multiply_bytes_grouped_device): job j
    is the sizes[j] bytes at arena_ptr + offsets[j], offsets[j] a multiple of 8.  Nothing outside a
    job's own bytes enters its value."""
    sizes, pres = [int(n) for n in sizes], [int(p) for p in pres]
    lv = _group_lefts(sizes, pres, lefts)
    out = np.zeros(sum(pres), np.uint64)
    of, nb, pr = _sizes(offsets), _sizes(sizes), _sizes(pres)
    _raise(N.load().lcpc_pos_left_multiply_bytes_grouped_device(
        arena_ptr, of.ctypes.data_as(N.szp), nb.ctypes.data_as(N.szp), pr.ctypes.data_as(N.szp), len(sizes), _p64(lv),
        lv.size, _p64(out), out.size))
    return _split_outputs(out, pres)


def left_multiply_group_plan(sizes, pres):
    """lcpc_pos_group_plan: (tiles, n_launches) for files of sizes[j] bytes with rows of pres[j]
    elements.  tiles is a structured array with the fields job, row_lo, row_hi, run_lo, run_hi, launch
    and wave: the work list of the grouped launches the calls above make, a job routed to the
    single-file path as one record with launch == GROUP_SINGLE.  Host only, a pure function."""
    nb, pr = _sizes(sizes), _sizes(pres)
    if nb.size != pr.size:
        raise ValueError("sizes and pres must have one entry per job")
    n, launches = C.c_size_t(), C.c_size_t()
    L = N.load()
    _raise(L.lcpc_pos_group_plan(nb.ctypes.data_as(N.szp), pr.ctypes.data_as(N.szp), nb.size, None, 0, C.byref(n),
                                 C.byref(launches)))
    dt = np.dtype([("job", "<u8"), ("row_lo", "<u8"), ("row_hi", "<u8"), ("run_lo", "<u8"), ("run_hi", "<u8"),
                   ("launch", "<u4"), ("wave", "<u4")])
    assert dt.itemsize == C.sizeof(N.PosGroupTile)
    tiles = np.zeros(n.value, dt)
    _raise(L.lcpc_pos_group_plan(nb.ctypes.data_as(N.szp), pr.ctypes.data_as(N.szp), nb.size,
                                 tiles.ctypes.data_as(C.POINTER(N.PosGroupTile)), tiles.size, C.byref(n),
                                 C.byref(launches)))
    return tiles, launches.value


def verify_group_plan(file_lens, pres, n_cols):
    """lcpc_pos_verify_group_plan: (tiles, n_launches) for audit responses over files of file_lens[j]
    bytes with rows of pres[j] elements and n_cols[j] opened columns.  tiles is a structured array with
    the fields job, col_lo, col_hi, chunk, launch and wave: the work list of the first launch of every
    staging group client_verify_evaluations_grouped makes, a job routed to the single sequence as one
    record per chunk with launch == GROUP_SINGLE.  Host only, a pure function."""
    nb, pr, nc = _sizes(file_lens), _sizes(pres), _sizes(n_cols)
    if not (nb.size == pr.size == nc.size):
        raise ValueError("file_lens, pres and n_cols must have one entry per job")
    n, launches = C.c_size_t(), C.c_size_t()
    L = N.load()
    args = (nb.ctypes.data_as(N.szp), pr.ctypes.data_as(N.szp), nc.ctypes.data_as(N.szp), nb.size)
    _raise(L.lcpc_pos_verify_group_plan(*args, None, 0, C.byref(n), C.byref(launches)))
    dt = np.dtype([("job", "<u8"), ("col_lo", "<u8"), ("col_hi", "<u8"), ("chunk", "<u8"), ("launch", "<u4"),
                   ("wave", "<u4")])
    assert dt.itemsize == C.sizeof(N.PosVerifyTile)
    tiles = np.zeros(n.value, dt)
    _raise(L.lcpc_pos_verify_group_plan(*args, tiles.ctypes.data_as(C.POINTER(N.PosVerifyTile)), tiles.size,
                                        C.byref(n), C.byref(launches)))
    return tiles, launches.value


def client_verify_evaluations_grouped(audits) -> list:
    """client_verify_evaluation for a queue of responses in one call
    (lcpc_pos_verify_evaluations_grouped): audits is a sequence of its argument tuples (root, file_len,
    pre, enc, point, cols, result_vector, columns).  Returns a list: entry i is the evaluation array
    client_verify_evaluation returns for audit i, word for word, or the VerifierError (ColumnEval) it
    would raise, as an instance that is not raised; its message names paths or values.  The launches are
    per staging group of responses, not per response.  The caller's own mistakes raise ValueError before
    any device work: non-increasing or out-of-range columns, dims the audits cannot have.  What the
    single check rejects from shapes alone (a wrong column count, a column that is not the file's row
    count long, a result vector that is not enc words, a digest that is not 32 bytes, paths of the
    wrong length) is that entry's VerifierError, and the job never reaches the library."""
    audits = list(audits)
    out: list = [None] * len(audits)
    jobs, keep, live = [], [], []
    for i, (root, file_len, pre, enc, point, cols, result_vector, columns) in enumerate(audits):
        file_len, pre, enc = int(file_len), int(pre), int(enc)
        idx = np.ascontiguousarray(np.asarray(list(cols), dtype=np.int64).reshape(-1))
        if idx.size > 1 and not (np.diff(idx) > 0).all():
            raise ValueError(f"audit {i}: requested columns must be strictly increasing")
        if file_len < 1 or pre < 1 or enc <= pre or enc & (enc - 1):
            raise ValueError(f"audit {i}: needs a non-empty file and enc a power of two > pre")
        if idx.size and (idx[0] < 0 or idx[-1] >= enc):
            raise ValueError(f"audit {i}: requested columns must be below enc")
        n_rows, plen = _file_rows(file_len, pre), enc.bit_length() - 1
        columns = list(columns)
        arrs = [np.asarray(c.col, dtype=np.uint64) for c in columns]
        if len(columns) != idx.size or {a.size for a in arrs} - {n_rows}:
            out[i] = _verifier_error("ColumnEval", "opened columns do not have the file's row count")
            continue
        res = np.ascontiguousarray(np.asarray(result_vector, dtype=np.uint64).reshape(-1))
        if res.size != enc:
            out[i] = _verifier_error("ColumnEval", "result vector is not one encoded row")
            continue
        if set(map(len, (c.path for c in columns))) - {plen}:
            out[i] = _verifier_error("ColumnEval", "Merkle paths of the wrong length")
            continue
        digests = list(itertools.chain.from_iterable(c.path for c in columns))
        rt = bytes(root)
        if len(rt) != 32 or set(map(len, digests)) - {32}:
            out[i] = _verifier_error("ColumnEval", "a path digest is not 32 bytes")
            continue
        paths = b"".join(digests)
        try:     # columns of one shape, (n_rows, 1) as a commitment opens them: one copy
            cm = np.concatenate(arrs) if arrs else np.zeros(0, np.uint64)
        except ValueError:
            cm = np.concatenate(arrs, axis=None)
        pb = np.frombuffer(paths, np.uint8) if paths else np.zeros(0, np.uint8)
        rb = np.frombuffer(rt, np.uint8)
        iu = idx.astype(np.uint64)
        x = int(np.asarray(point, dtype=np.uint64).reshape(-1)[0])
        keep.append((cm, pb, rb, iu, res))
        jobs.append(N.PosAuditJob(rb.ctypes.data, file_len, pre, enc, x, iu.ctypes.data if iu.size else None,
                                  iu.size, cm.ctypes.data if iu.size else None, pb.ctypes.data if iu.size else None,
                                  res.ctypes.data))
        live.append(i)
    if not jobs:
        return out
    arr = (N.PosAuditJob * len(jobs))(*jobs)
    verdict = np.zeros(len(jobs), np.uint8)
    values = np.zeros(len(jobs), np.uint64)
    _raise(N.load().lcpc_pos_verify_evaluations_grouped(arr, len(jobs), verdict.ctypes.data_as(N.u8p), _p64(values)))
    del keep
    for k, i in enumerate(live):
        if verdict[k] == 0:
            out[i] = values[k:k + 1].reshape(1, 1).copy()
        elif verdict[k] == 1:
            out[i] = _verifier_error("ColumnEval", "Merkle path mismatch (paths)")
        else:
            out[i] = _verifier_error("ColumnEval", "column value mismatch (values)")
    return out


# ---------------------------------------------------------------- grouped ingest of small files
INGEST_MAX_ENC = 1024            # LCPC_POS_INGEST_MAX_ENC: rows of more points take the single path
INGEST_TILE_ROWS = 8             # LCPC_POS_INGEST_TILE_ROWS
INGEST_LAUNCHES_PER_GROUP = 3    # LCPC_POS_INGEST_LAUNCHES_PER_GROUP
DIGEST_BYTES = 32


def _job_rows(n_bytes: int, pre: int) -> int:
    return -(-(-(-n_bytes // DATA_BYTE_CAPACITY)) // pre)


def _leaf_chunks(rows: int) -> int:
    return (32 + WRITTEN_BYTES_WIDTH * rows + 1023) // 1024


def _row_plan(entry, columns):
    """the size-then-fill calls of lcpc_pos_ingest_plan, lcpc_pos_scrub_plan and lcpc_pos_repair_plan
    (entry) over the per-job size arrays `columns`: (tiles, n_groups)"""
    n, launches = C.c_size_t(), C.c_size_t()
    args = tuple(a.ctypes.data_as(N.szp) for a in columns) + (columns[0].size,)
    _raise(entry(*args, None, 0, C.byref(n), C.byref(launches)))
    dt = np.dtype([("job", "<u8"), ("row_lo", "<u8"), ("row_hi", "<u8"), ("launch", "<u4"), ("workgroup", "<u4")])
    assert dt.itemsize == C.sizeof(N.PosIngestTile)
    tiles = np.zeros(n.value, dt)
    _raise(entry(*args, tiles.ctypes.data_as(C.POINTER(N.PosIngestTile)), tiles.size, C.byref(n), C.byref(launches)))
    return tiles, launches.value


def ingest_plan(n_bytes, pres, encs):
    """lcpc_pos_ingest_plan: (tiles, n_groups) for files of n_bytes[j] bytes at dims pres[j] / encs[j].
    tiles is a structured array with the fields job, row_lo, row_hi, launch and workgroup: the work list
    of the encode launch of every staging group encode_files_grouped makes (launch = the group), a job
    routed to the single-file path as one record with launch == GROUP_SINGLE.  Host only, a pure function."""
    nb, pr, en = _sizes(n_bytes), _sizes(pres), _sizes(encs)
    if not (nb.size == pr.size == en.size):
        raise ValueError("n_bytes, pres and encs must have one entry per job")
    return _row_plan(N.load().lcpc_pos_ingest_plan, (nb, pr, en))


def _addr(a):
    """the address of an array's first byte, None for no array or an empty one"""
    return a.ctypes.data if a is not None and a.size else None


def _per_job(value, n: int) -> list:
    return [bool(value)] * n if isinstance(value, (bool, np.bool_)) else [bool(v) for v in value]


def encode_files_grouped_into(datas, pres, encs, porencs=None, row_capacities=None, want_tree=True, want_root=False,
                              want_cvs=False):
    """lcpc_pos_encode_files_grouped over caller buffers: job j encodes datas[j] (bytes or a uint8 array, at
    any address) at pres[j] / encs[j] into porencs[j], a writable contiguous uint8 / uint64 array that holds a
    column-major image of row_capacities[j] rows (None: no image for that job; porencs=None: for no job, and
    then no encoded word leaves the device).  want_tree / want_root / want_cvs: a bool or one per job.
    Returns a list of dicts with rows_written and, where asked, tree ((2 enc - 1, 32) uint8), root (bytes)
    and cvs ((chunks, enc, 32) uint8).  Rows of an image past rows_written are not touched."""
    images = [_as_image(d) for d in datas]
    n = len(images)
    pres, encs = [int(p) for p in pres], [int(e) for e in encs]
    if not (len(pres) == len(encs) == n):
        raise ValueError("datas, pres and encs must have one entry per job")
    porencs = [None] * n if porencs is None else list(porencs)
    caps = [0] * n if row_capacities is None else [int(c) for c in row_capacities]
    if not (len(porencs) == len(caps) == n):
        raise ValueError("porencs and row_capacities must have one entry per job")
    trees_on, roots_on, cvs_on = _per_job(want_tree, n), _per_job(want_root, n), _per_job(want_cvs, n)
    jobs, out = [], []
    for j in range(n):
        pre, enc = pres[j], encs[j]
        ok = pre >= 1 and enc > pre
        rows = _job_rows(images[j].size, pre) if ok else 0
        o = {"rows_written": 0}
        if trees_on[j] and ok:
            o["tree"] = np.zeros((2 * enc - 1, DIGEST_BYTES), np.uint8)
        if roots_on[j]:
            o["root"] = np.zeros(DIGEST_BYTES, np.uint8)
        if cvs_on[j] and ok:
            o["cvs"] = np.zeros((_leaf_chunks(rows), enc, DIGEST_BYTES), np.uint8)
        img = porencs[j]
        if img is not None:
            if not (isinstance(img, np.ndarray) and img.flags.c_contiguous and img.flags.writeable):
                raise ValueError("a porenc must be a writable contiguous array")
            if img.nbytes < caps[j] * enc * WRITTEN_BYTES_WIDTH:
                raise ValueError("a porenc is smaller than row_capacity x enc elements")
        jobs.append(N.PosIngestJob(_addr(images[j]), images[j].size, pre, enc,
                                   img.ctypes.data if img is not None else None, caps[j], _addr(o.get("tree")),
                                   _addr(o.get("root")), _addr(o.get("cvs")), 0))
        out.append(o)
    arr = (N.PosIngestJob * max(n, 1))(*jobs)
    _raise(N.load().lcpc_pos_encode_files_grouped(arr if n else None, n))
    for j, o in enumerate(out):
        o["rows_written"] = int(arr[j].rows_written)
        if "root" in o:
            o["root"] = o["root"].tobytes()
    del images
    return out


def encode_files_grouped(datas, pres, encs, want_porenc: bool = True, want_cvs: bool = False):
    """The stored form of many files in one call (lcpc_pos_encode_files_grouped): per file a tuple
    (image, tree, rows_written[, cvs]) -- image the written rows of the column-major `.porenc` as an
    (enc, rows_written) uint64 array (None without want_porenc), tree the (2 enc - 1, 32) digests of the
    `.portree`, cvs the [chunk][column] chaining values of the `.porcv` sidecar -- each byte for byte what
    one lcpc_pos_encode_file per file gives, with a number of launches that does not grow with the number
    of files (files whose rows have more than INGEST_MAX_ENC points take that path inside the call)."""
    images = [_as_image(d) for d in datas]
    pres, encs = [int(p) for p in pres], [int(e) for e in encs]
    porencs = caps = None
    if want_porenc:
        caps = [_job_rows(a.size, p) if p >= 1 else 0 for a, p in zip(images, pres)]
        porencs = [np.zeros((e, c), np.uint64) for e, c in zip(encs, caps)]
    res = encode_files_grouped_into(images, pres, encs, porencs, caps, True, False, want_cvs)
    out = []
    for j, o in enumerate(res):
        t = (porencs[j] if want_porenc else None, o["tree"], o["rows_written"])
        out.append(t + (o["cvs"],) if want_cvs else t)
    return out


def commit_roots_of_files(datas, pres, encs) -> List[bytes]:
    """The Merkle root of every file's stored form (RowGeneratorIter.convert_to_commit_root per file) in
    one grouped call; no encoded word is copied back from the device."""
    res = encode_files_grouped_into(datas, pres, encs, None, None, False, True, False)
    return [o["root"] for o in res]


# ---------------------------------------------------------------- grouped scrub of stored files
SCRUB_MAX_ENC = 1024             # LCPC_POS_SCRUB_MAX_ENC: rows of more points take the single-file entries
SCRUB_TILE_ROWS = 8              # LCPC_POS_SCRUB_TILE_ROWS
SCRUB_LAUNCHES_PER_GROUP = 3     # LCPC_POS_SCRUB_LAUNCHES_PER_GROUP
_SCRUB_NOT_EVALUATED = 0xFF      # LCPC_POS_SCRUB_NOT_EVALUATED
_SCRUB_ROWS_UNCHECKED = (1 << (8 * C.sizeof(C.c_size_t))) - 1   # LCPC_POS_SCRUB_ROWS_UNCHECKED


def scrub_plan(rows_written, pres, encs):
    """lcpc_pos_scrub_plan: (tiles, n_groups) for stored files of rows_written[j] rows at dims pres[j] /
    encs[j].  tiles is a structured array with the fields job, row_lo, row_hi, launch and workgroup: the
    work list of the row-check launch of every staging group scrub_files_grouped makes (launch = the
    group), a job routed to the single-file entries as one record with launch == GROUP_SINGLE.  Host
    only, a pure function."""
    rw, pr, en = _sizes(rows_written), _sizes(pres), _sizes(encs)
    if not (rw.size == pr.size == en.size):
        raise ValueError("rows_written, pres and encs must have one entry per job")
    return _row_plan(N.load().lcpc_pos_scrub_plan, (rw, pr, en))


def _byte_view(data) -> np.ndarray:
    """the bytes of a stored image (an array of any dtype, an mmap, bytes) without a copy where it is contiguous"""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    return np.frombuffer(data, np.uint8)


def scrub_files_grouped(images, pres, encs, rows_written, row_capacities, trees=None, expected_roots=None,
                        want_digests: bool = False) -> list:
    """lcpc_pos_scrub_files_grouped: the triage of many stored files in one call.  Job j is the column-major
    `.porenc` image images[j] (a numpy array or an mmap of row_capacities[j] x encs[j] elements, None with no
    rows) of which rows_written[j] rows count, trees[j] its stored digests (None, the encs[j] leaves, or the
    whole 2 enc - 1 `.portree`, as bytes or a uint8 array) and expected_roots[j] the root its owner holds
    (32 bytes or None).  Returns one dict per job: status ((enc,) uint8: 0 the column's digest equals its
    stored leaf, 1 it differs, 2 it holds an element that is not < p; without a tree 0 or 2 only), digests
    ((enc, 32) uint8 with want_digests, else None), n_bad, n_dirty_rows (the rows that are no codewords of
    the row code; None where a status-2 column leaves them unchecked), tree_consistent and root_ok (None
    where there is nothing to evaluate).  Status, digests and n_bad are those of lcpc_pos_scrub_porenc and
    n_dirty_rows that of lcpc_pos_locate_porenc per file; the launches are per staging group of files."""
    n = len(images)
    pres, encs = [int(p) for p in pres], [int(e) for e in encs]
    rows, caps = [int(r) for r in rows_written], [int(c) for c in row_capacities]
    trees = [None] * n if trees is None else list(trees)
    roots = [None] * n if expected_roots is None else list(expected_roots)
    if not (len(pres) == len(encs) == len(rows) == len(caps) == len(trees) == len(roots) == n):
        raise ValueError("every argument must have one entry per job")
    jobs, keep, out = [], [], []
    for j in range(n):
        enc = encs[j]
        img = None if images[j] is None else _byte_view(images[j])
        if img is not None and img.size < caps[j] * enc * WRITTEN_BYTES_WIDTH:
            raise ValueError(f"job {j}: the image is smaller than row_capacity x enc elements")
        tree = None if trees[j] is None else _byte_view(trees[j])
        if tree is not None and tree.size % DIGEST_BYTES:
            raise ValueError(f"job {j}: a tree is whole 32-byte digests")
        root = None if roots[j] is None else np.frombuffer(bytes(roots[j]), np.uint8)
        if root is not None and root.size != DIGEST_BYTES:
            raise ValueError(f"job {j}: an expected root is 32 bytes")
        status = np.zeros(max(enc, 0), np.uint8)
        digests = np.zeros((max(enc, 0), DIGEST_BYTES), np.uint8) if want_digests else None
        keep.append((img, tree, root))
        jobs.append(N.PosScrubJob(_addr(img), pres[j], enc, rows[j], caps[j], _addr(tree),
                                  tree.size // DIGEST_BYTES if tree is not None else 0, _addr(root),
                                  status.ctypes.data if status.size else None, _addr(digests), 0, 0, 0, 0))
        out.append({"status": status, "digests": digests})
    arr = (N.PosScrubJob * max(n, 1))(*jobs)
    _raise(N.load().lcpc_pos_scrub_files_grouped(arr if n else None, n))
    del keep

    def flag(v):
        return None if v == _SCRUB_NOT_EVALUATED else bool(v)
    for j, o in enumerate(out):
        o["n_bad"] = int(arr[j].n_bad)
        nd = int(arr[j].n_dirty_rows)
        o["n_dirty_rows"] = None if nd == _SCRUB_ROWS_UNCHECKED else nd
        o["tree_consistent"] = flag(arr[j].tree_consistent)
        o["root_ok"] = flag(arr[j].root_ok)
    return out


# ---------------------------------------------------------------- grouped repair of stored files
REPAIR_MAX_ENC = 1024             # LCPC_POS_REPAIR_MAX_ENC: rows of more points take lcpc_pos_repair_columns
REPAIR_TILE_ROWS = 8              # LCPC_POS_REPAIR_TILE_ROWS
REPAIR_LAUNCHES_PER_GROUP = 4     # LCPC_POS_REPAIR_LAUNCHES_PER_GROUP


def repair_plan(rows_written, pres, encs, n_bad):
    """lcpc_pos_repair_plan: (tiles, n_groups) for stored files of rows_written[j] rows at dims pres[j] /
    encs[j] with n_bad[j] listed columns.  tiles is a structured array with the fields job, row_lo, row_hi,
    launch and workgroup: the work list of the row launch of every staging group repair_files_grouped makes
    (launch = the group), a job routed to lcpc_pos_repair_columns as one record with launch ==
    GROUP_SINGLE; a job with more listed columns than encs[j] - pres[j], or with no rows, has no record.
    Host only, a pure function."""
    rw, pr, en, nb = _sizes(rows_written), _sizes(pres), _sizes(encs), _sizes(n_bad)
    if not (rw.size == pr.size == en.size == nb.size):
        raise ValueError("rows_written, pres, encs and n_bad must have one entry per job")
    return _row_plan(N.load().lcpc_pos_repair_plan, (rw, pr, en, nb))


def repair_files_grouped(images, pres, encs, rows_written, row_capacities, bad_cols, leaves=None,
                         want_cols: bool = True, want_tree: bool = False) -> list:
    """lcpc_pos_repair_files_grouped: the listed columns of many stored files recomputed in one call.  Job j
    is the column-major `.porenc` image images[j] (a numpy array or an mmap of row_capacities[j] x encs[j]
    elements, None with no rows) of which rows_written[j] rows count, bad_cols[j] its erasure set (distinct
    columns, never read from the image) and leaves[j] the encs[j] digests of its columns as they stand
    (bytes or a uint8 array, or None).  Returns one dict per job: status (0, or UNRECOVERABLE when the job
    lists more than enc - pre columns, a row is no codeword on the columns that are not listed, or one of
    them holds a word that is not < p), cols ((n_bad, rows_written) uint64 with want_cols), digests ((n_bad,
    32) uint8), tree ((2 enc - 1, 32) uint8: the tree over the leaves with the repaired digests in place)
    and root (bytes) with want_tree for a job with leaves.  The data of a failed job is None.  Every answer
    is byte for byte lcpc_pos_repair_columns' per file; the launches are per staging group of files."""
    n = len(images)
    pres, encs = [int(p) for p in pres], [int(e) for e in encs]
    rows, caps = [int(r) for r in rows_written], [int(c) for c in row_capacities]
    leaves = [None] * n if leaves is None else list(leaves)
    bad_cols = list(bad_cols)
    if not (len(pres) == len(encs) == len(rows) == len(caps) == len(bad_cols) == len(leaves) == n):
        raise ValueError("every argument must have one entry per job")
    jobs, keep, out = [], [], []
    for j in range(n):
        enc = encs[j]
        img = None if images[j] is None else _byte_view(images[j])
        if img is not None and img.size < caps[j] * enc * WRITTEN_BYTES_WIDTH:
            raise ValueError(f"job {j}: the image is smaller than row_capacity x enc elements")
        bad = np.ascontiguousarray(np.asarray(bad_cols[j], np.uint64).reshape(-1))
        lv = None if leaves[j] is None else _byte_view(leaves[j])
        if lv is not None and lv.size != max(enc, 0) * DIGEST_BYTES:
            raise ValueError(f"job {j}: the leaves are enc 32-byte digests")
        nb = int(bad.size)
        cols = np.zeros((nb, rows[j]), np.uint64) if want_cols else None
        digests = np.zeros((nb, DIGEST_BYTES), np.uint8)
        tree = np.zeros((2 * enc - 1, DIGEST_BYTES), np.uint8) if want_tree and lv is not None and enc >= 1 else None
        root = np.zeros(DIGEST_BYTES, np.uint8) if tree is not None else None
        keep.append((img, bad, lv))
        jobs.append(N.PosRepairJob(_addr(img), pres[j], enc, rows[j], caps[j], _addr(bad), nb, _addr(lv),
                                   _addr(cols), _addr(digests), _addr(tree), _addr(root), 0))
        out.append({"cols": cols, "digests": digests, "tree": tree, "root": root})
    arr = (N.PosRepairJob * max(n, 1))(*jobs)
    _raise(N.load().lcpc_pos_repair_files_grouped(arr if n else None, n))
    del keep
    for j, o in enumerate(out):
        o["status"] = int(arr[j].status)
        if o["status"]:
            o["cols"] = o["digests"] = o["tree"] = o["root"] = None
        elif o["root"] is not None:
            o["root"] = o["root"].tobytes()
    return out


# ---------------------------------------------------------------- grouped locate of stored files
LOCATE_MAX_ENC = 1024             # LCPC_POS_LOCATE_MAX_ENC: rows of more points take lcpc_pos_locate_porenc
LOCATE_LAUNCHES_PER_GROUP = 4     # LCPC_POS_LOCATE_LAUNCHES_PER_GROUP
LOCATE_ROW_NOT_EVALUATED = 0xFF   # LCPC_POS_LOCATE_ROW_NOT_EVALUATED


def locate_files_grouped(images, pre, enc, rows_written, row_capacity, known_bad=None,
                         want_row_status: bool = False) -> list:
    """lcpc_pos_locate_files_grouped: the damaged columns of many stored files named by their own rows
    (syndromes, Berlekamp-Massey, a root search) in one call.  Job j is the column-major `.porenc` image
    images[j] (a numpy array or an mmap of row_capacity[j] x enc[j] elements, None with no rows) of which
    rows_written[j] rows count and known_bad[j] the columns already known to be bad (distinct, never read
    from the image; None for none).  Returns one dict per job: status (0, or UNRECOVERABLE when the known
    columns and those holding a word that is not < p exceed enc - pre), col_status ((enc,) uint8: 0 sound,
    1 some row located a wrong element there, 2 it holds a word that is not < p, 3 listed), n_bad_cols,
    n_dirty_rows (rows that are no codewords), n_unlocatable_rows (of those, the rows that cannot name
    their wrong positions) and row_status ((rows_written,) uint8 with want_row_status: 0 / 1 / 2, or
    LOCATE_ROW_NOT_EVALUATED throughout for a job the single-file entry answered).  The data of a failed
    job is None.  col_status, the counters and status are byte for byte lcpc_pos_locate_porenc's per file;
    the launches are per staging group of files (the grouped repair's groups with known_bad as its list:
    repair_plan(rows_written, pre, enc, [len(k) for k in known_bad]) is the work list)."""
    n = len(images)
    pres, encs = [int(p) for p in pre], [int(e) for e in enc]
    rows, caps = [int(r) for r in rows_written], [int(c) for c in row_capacity]
    known_bad = [None] * n if known_bad is None else list(known_bad)
    if not (len(pres) == len(encs) == len(rows) == len(caps) == len(known_bad) == n):
        raise ValueError("every argument must have one entry per job")
    jobs, keep, out = [], [], []
    for j in range(n):
        e = encs[j]
        img = None if images[j] is None else _byte_view(images[j])
        if img is not None and img.size < caps[j] * e * WRITTEN_BYTES_WIDTH:
            raise ValueError(f"job {j}: the image is smaller than row_capacity x enc elements")
        kb = np.zeros(0, np.uint64) if known_bad[j] is None else \
            np.ascontiguousarray(np.asarray(known_bad[j], np.uint64).reshape(-1))
        col_status = np.zeros(max(e, 1), np.uint8)
        row_status = np.zeros(max(rows[j], 1), np.uint8) if want_row_status else None
        keep.append((img, kb))
        jobs.append(N.PosLocateJob(_addr(img), pres[j], e, rows[j], caps[j], _addr(kb) if kb.size else None,
                                   int(kb.size), _addr(col_status), _addr(row_status), 0, 0, 0, 0))
        out.append({"col_status": col_status[:max(e, 0)],
                    "row_status": row_status[:rows[j]] if want_row_status else None})
    arr = (N.PosLocateJob * max(n, 1))(*jobs)
    _raise(N.load().lcpc_pos_locate_files_grouped(arr if n else None, n))
    del keep
    for j, o in enumerate(out):
        o["status"] = int(arr[j].status)
        o["n_bad_cols"] = int(arr[j].n_bad_cols)
        o["n_dirty_rows"] = int(arr[j].n_dirty_rows)
        o["n_unlocatable_rows"] = int(arr[j].n_unlocatable_rows)
        if o["status"]:
            o["col_status"] = o["row_status"] = o["n_bad_cols"] = o["n_dirty_rows"] = o["n_unlocatable_rows"] = None
    return out


def field_to_montgomery(values, field: int = FT63) -> np.ndarray:
    """lcpc_field_to_montgomery: (v R) mod p per 64-bit word, R = 2^64 (Ft63 only): canonical values,
    as a `.porenc` holds them, to the Montgomery words a commitment opens.  Same shape as `values`."""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    out = np.empty_like(a)
    _raise(N.load().lcpc_field_to_montgomery(field, _p64(a.reshape(-1)), _p64(out.reshape(-1)), a.size))
    return out


def client_verify_batch_evaluation(root: bytes, file_len: int, pre: int, enc: int, points, vectors, column_indices,
                                   columns: Sequence[LcColumn]) -> np.ndarray:
    """One audit of a stored file at m points: `vectors` (m, pre) are the server's unencoded vectors
    v_j = left_j^T M (FileHandler.batch_evaluation_vectors), `columns` the opened columns with their
    paths for `column_indices` (Montgomery limbs, as a commitment opens them).  Checks, as
    _checked_file_evaluation does for one point: the indices are strictly increasing (ValueError),
    every column has the file's row count, every path leads to root, every word of `vectors` is
    below p, and Enc(v_j)[idx_k] == <left_j, col_k> for every (j, k) -- one encode of the m rows and
    one many-tensor combination of the k columns.  Returns the m evaluations <v_j, right_j>, (m, 1);
    raises VerifierError(ColumnEval) otherwise.

    ORDER IS A SOUNDNESS CONDITION: the client must hold all m vectors before it reveals
    column_indices.  A server that knows the k < pre columns it will be checked on can fit a false
    vector to exactly those positions; fixed before the draw, a false v_j differs from the true one
    in at least enc - pre + 1 positions of its encoding and survives the k openings with the
    probability it has in a single audit.  The batch is no weaker than the weakest of its m single
    audits (the stored-file form of lcpc_prove_batch absorbing every p_eval_j before the columns)."""
    cols = [int(c) for c in column_indices]
    if any(b <= a for a, b in zip(cols, cols[1:])):
        raise ValueError("requested columns must be strictly increasing")
    n_rows = _file_rows(file_len, pre)
    if len(columns) != len(cols) or any(np.asarray(c.col).size != n_rows for c in columns):
        raise _verifier_error("ColumnEval", "opened columns do not have the file's row count")
    if any(not 0 <= c < enc for c in cols):
        raise _verifier_error("ColumnEval", "column index outside the encoded row")
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64)).reshape(-1)
    m = pts.size
    v = np.asarray(vectors, dtype=np.uint64)
    if m == 0 or v.size != m * pre:
        raise _verifier_error("ColumnEval", "vectors are not one unencoded row per point")
    v = np.ascontiguousarray(v.reshape(m, pre))
    if (v >= np.uint64(FT63_MODULUS)).any():
        raise _verifier_error("ColumnEval", "vector word not below the modulus")
    client_online_verify_column_paths(root, cols, columns)
    sides = [form_side_vectors_for_polynomial_evaluation_from_point(pts[j:j + 1], n_rows, pre) for j in range(m)]
    lefts = np.stack([l.reshape(-1) for l, _ in sides])
    rights = np.stack([r.reshape(-1) for _, r in sides])
    rows = np.zeros((m, enc, 1), np.uint64)
    rows[:, :pre, 0] = v
    encoded = LigeroEncoding.new_from_dims(FT63, pre, enc).encode_rows(rows).reshape(m, enc)
    if cols:
        opened = np.ascontiguousarray(np.stack([np.asarray(c.col, dtype=np.uint64).reshape(-1) for c in columns], axis=1))
        dots = collapse_columns_many(FT63, opened, lefts, n_rows, len(cols)).reshape(m, len(cols))
        if not np.array_equal(dots, encoded[:, cols]):
            raise _verifier_error("ColumnEval", "column value mismatch")
    # <v_j, right_j>: the diagonal of one many-tensor combination of the vectors against the rights
    vals = collapse_columns_many(FT63, np.ascontiguousarray(v.T), rights, pre, m).reshape(m, m)
    return np.ascontiguousarray(np.diagonal(vals)).reshape(m, 1)

