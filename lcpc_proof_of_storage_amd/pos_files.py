"""Proof-of-storage encoded files over liblcpc_mi.so: the `.porenc` / `.portree` / `.meta`
formats of the reference's proof-of-storage/src/lcpc_online (names kept):

  EncodedFileWriter     encoded_file_writer.rs:24-501  (new, push_bytes, finalize_*,
                        convert_unencoded_file, get_encoded_file_metadata)
  EncodedFileReader     encoded_file_reader.rs:20-381  (get_encoded_row,
                        get_encoded_column_without_path, get_unencoded_row[_bytes],
                        decode_to_target_file, process_file_to_merkle_tree, set_new_capacity,
                        resize_to_target_file, get_unencoded_file_len)
  EncodedFileMetadata   encoded_file_metadata.rs:6-27  (serde_json)
  MerkleTree            merkle_tree.rs:7-86             (digests = leaves || parents)
  read_tree / write_tree_to_file                         file_handler.rs:714-735
  get_encoded_file_size_from_rate / get_decoded_file_size_from_rate   reader.rs:384-407
  RowGeneratorIter      row_generator_iter.rs:8-165     (new_ligero, next, get_column_digests,
                        get_specified_column_digests, convert_to_commit_root, get_full_columns)
  ColumnDigestAccumulator, ColumnsToCareAbout   column_digest_accumulator.rs:9-118
  ColumnChunkCache, the `.porcv` sidecar          no counterpart: incremental Merkle updates
                        (FileHandler(chunk_cache=True)), same trees and files as without it
  ScrubReport, UnrecoverableError, FileHandler.scrub / repair,
  EncodedFileReader.find_damaged_columns / repair_columns / decode_with_erasures
                        no counterpart: damaged columns located against the stored leaves and
                        recomputed by Reed-Solomon erasure decoding
  EncodedFileReader.locate_damaged_columns, FileHandler.scrub / repair (locate=True)
                        no counterpart: damaged columns located by the code's own syndromes where
                        the tree cannot say

Layout of a `.porenc` file (WriteableFt63): column c occupies row_capacity * 8 bytes starting at
byte c * row_capacity * 8; its first rows_written elements are the canonical little-endian repr
of the encoded matrix's column c, the rest zero.  The writer starts with row_capacity = 2 * rows
and doubles it when rows reach it.

Every byte of encoding, hashing and decoding runs on the GPU (liblcpc_mi.so); this module maps
the files and hands the library pointers into them.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import mmap
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _native as N
from . import lcpc2d as L
from .lcpc2d import _raise

WRITTEN_BYTES_WIDTH = 8   # size_of::<WriteableFt63>() (data_field.rs:24)
DATA_BYTE_CAPACITY = 7    # CAPACITY / 8 (data_field.rs:22)
DIGEST_BYTES = 32
_NULL_ULID = "0" * 26     # Ulid::default() as serialized by the ulid crate's serde impl


def _u8(a: np.ndarray):
    return a.ctypes.data_as(N.u8p) if a.size else None


def _bytes_ptr(b) -> Tuple[Optional[C.POINTER(C.c_uint8)], object]:
    arr = np.frombuffer(b, dtype=np.uint8) if len(b) else np.zeros(0, np.uint8)
    return _u8(arr), arr


# ---------------------------------------------------------------- scrub / repair results
LCPC_ERR_UNRECOVERABLE = 36


class UnrecoverableError(Exception):
    """More columns are damaged than the code's redundancy covers (or what was recomputed does not
    verify against the trust anchor), and no other copy helps.  FileHandler.repair leaves every
    file as it was when it raises this."""


@dataclass
class ScrubReport:
    """What FileHandler.scrub found (repair returns the same for the state it met, with
    repaired_from saying what it then did)."""
    bad_columns: List[int]            # `.porenc` columns whose digest differs from their stored leaf
    noncanonical_columns: List[int]   # those among them that hold an element that is not < p
    tree_consistent: bool             # the stored tree's leaves refold to its parents and root
    root_ok: Optional[bool]           # stored root == expected_root (None: no expected_root given)
    raw_ok: bool                      # the raw file re-encodes to the stored tree
    repaired_from: Optional[str] = None  # repair: "+"-joined of "columns", "tree", "reencode", "raw"
    # locate=True only: the columns the code's own syndromes name (no tree needed), and the rows whose
    # wrong elements are too many to be located
    located_columns: Optional[List[int]] = None
    unlocatable_rows: Optional[int] = None

    @property
    def clean(self) -> bool:
        return not self.bad_columns and self.tree_consistent and self.root_ok is not False and self.raw_ok


# ---------------------------------------------------------------- metadata / Merkle tree
@dataclass
class EncodedFileMetadata:
    """encoded_file_metadata.rs:6-13 (serde_json, field order kept)."""
    pre_encoded_size: int
    encoded_size: int
    rows_written: int
    row_capacity: int
    bytes_of_data: int
    ulid: str = _NULL_ULID

    def to_json(self) -> str:
        return json.dumps({"ulid": self.ulid, "pre_encoded_size": self.pre_encoded_size,
                           "encoded_size": self.encoded_size, "rows_written": self.rows_written,
                           "row_capacity": self.row_capacity, "bytes_of_data": self.bytes_of_data},
                          separators=(",", ":"))

    def write_to_file(self, writable) -> None:
        writable.write(self.to_json().encode())

    @classmethod
    def read_from_file(cls, readable) -> "EncodedFileMetadata":
        d = json.loads(readable.read())
        return cls(d["pre_encoded_size"], d["encoded_size"], d["rows_written"], d["row_capacity"],
                   d["bytes_of_data"], d.get("ulid", _NULL_ULID))


class MerkleTree:
    """merkle_tree.rs:7-86: 2 w - 1 digests, the w leaves then every parent level, root last."""

    def __init__(self, digests: np.ndarray):
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1, DIGEST_BYTES)
        self.digests = d
        self.width = (d.shape[0] + 1) // 2

    @classmethod
    def new(cls, children_leaves) -> "MerkleTree":
        leaves = np.ascontiguousarray(np.frombuffer(bytes(children_leaves), np.uint8)
                                      if isinstance(children_leaves, (bytes, bytearray))
                                      else children_leaves, dtype=np.uint8).reshape(-1, DIGEST_BYTES)
        w = leaves.shape[0]
        if w < 2 or w & (w - 1):
            raise ValueError("Input needs to be a power of two, at least two.")
        d = np.zeros((2 * w - 1, DIGEST_BYTES), np.uint8)
        d[:w] = leaves
        _raise(N.load().lcpc_merkle_tree(_u8(d[:w]), w, _u8(d[w:])))
        return cls(d)

    def root(self) -> bytes:
        return self.digests[-1].tobytes()

    def get_path(self, index: int) -> Optional[List[bytes]]:
        if index >= self.width:
            return None
        path, base, level_len = [], 0, self.width
        while level_len > 1:
            path.append(self.digests[base + (index ^ 1)].tobytes())
            base += level_len
            level_len //= 2
            index >>= 1
        return path

    def __len__(self) -> int:
        return self.digests.shape[0]

    def __getitem__(self, i: int) -> bytes:
        return self.digests[i].tobytes()

    def __eq__(self, other) -> bool:
        return isinstance(other, MerkleTree) and np.array_equal(self.digests, other.digests)

    def to_bytes(self) -> bytes:
        return self.digests.tobytes()

    @classmethod
    def from_bytes(cls, data: bytes) -> "MerkleTree":
        n = len(data) // DIGEST_BYTES
        if (n + 1) & n:
            raise ValueError("input size must be a power of two")
        if n <= 2:
            raise ValueError("Merkle tree must be a non-trivial binary tree")
        return cls(np.frombuffer(data[:n * DIGEST_BYTES], np.uint8).copy())


def read_tree(tree_file) -> MerkleTree:
    tree_file.seek(0)
    return MerkleTree.from_bytes(tree_file.read())


def write_tree_to_file(tree_file, tree: MerkleTree) -> None:
    tree_file.write(tree.to_bytes())


def get_encoded_file_size_from_rate(decoded_file_size: int, pre_encoded_len: int, encoded_len: int) -> int:
    """reader.rs:384-395 (div_ceils first, in this order)."""
    return (-(-(-(-decoded_file_size // DATA_BYTE_CAPACITY)) // pre_encoded_len)
            * WRITTEN_BYTES_WIDTH * encoded_len)


def get_decoded_file_size_from_rate(encoded_file_size: int, pre_encoded_len: int, encoded_len: int) -> int:
    """reader.rs:397-407."""
    return (-(-(-(-encoded_file_size // encoded_len)) // WRITTEN_BYTES_WIDTH)
            * DATA_BYTE_CAPACITY * pre_encoded_len)


# ---------------------------------------------------------------- column chunk-CV cache
# A column digest is BLAKE3(32 zero bytes || the column's elements): a tree over 1-KiB chunks whose
# chaining values (CVs) depend only on the chunk's bytes, its counter and whether it is the only
# chunk.  Keeping them ([chunk][column] x 32 B) makes an edit or append rehash only the chunks it
# touched ("Incremental Merkle updates").  The `.porcv` sidecar stores them next to the
# reference's four files: a 64-byte header, then the CVs.
CHUNK_CV_EXTENSION = "porcv"
CHUNK_CV_MAGIC = b"PORCV\x00\x00\x01"   # 8 bytes: name and format version 1
CHUNK_CV_HEADER_BYTES = 64
CHUNK_BYTES, CV_BYTES = 1024, 32


def leaf_n_chunks(rows_written: int) -> int:
    """1-KiB chunks of a column message of rows_written elements (the empty message has one)."""
    return max(1, -(-(DIGEST_BYTES + rows_written * WRITTEN_BYTES_WIDTH) // CHUNK_BYTES))


def encode_chunk_cv_header(enc: int, rows_written: int, n_chunks: int, root: bytes) -> bytes:
    """magic/version, u64 LE enc, rows_written, n_chunks, the 32-byte root the CVs fold to."""
    if len(root) != DIGEST_BYTES:
        raise ValueError("root must be 32 bytes")
    return (CHUNK_CV_MAGIC + enc.to_bytes(8, "little") + rows_written.to_bytes(8, "little")
            + n_chunks.to_bytes(8, "little") + bytes(root))


def parse_chunk_cv_header(header: bytes) -> Tuple[int, int, int, bytes]:
    """(enc, rows_written, n_chunks, root); ValueError on a short header or another magic."""
    if len(header) < CHUNK_CV_HEADER_BYTES:
        raise ValueError("chunk-CV sidecar shorter than its header")
    if header[:8] != CHUNK_CV_MAGIC:
        raise ValueError("not a chunk-CV sidecar (magic / version)")
    enc, rows, n_chunks = (int.from_bytes(header[8 + 8 * i:16 + 8 * i], "little") for i in range(3))
    return enc, rows, n_chunks, bytes(header[32:64])


def check_chunk_cv_sidecar(header: bytes, file_len: int, enc: int, rows_written: int, root: bytes) -> int:
    """The sidecar's n_chunks if its header matches the file's metadata (enc, rows_written), its
    length holds every CV and its root is the stored tree's; ValueError otherwise."""
    h_enc, h_rows, h_chunks, h_root = parse_chunk_cv_header(header)
    if (h_enc, h_rows) != (enc, rows_written) or h_chunks != leaf_n_chunks(rows_written):
        raise ValueError("chunk-CV sidecar is for other dimensions")
    if file_len < CHUNK_CV_HEADER_BYTES + h_chunks * h_enc * CV_BYTES:
        raise ValueError("chunk-CV sidecar body is short")
    if h_root != bytes(root):
        raise ValueError("chunk-CV sidecar root differs from the stored tree's")
    return h_chunks


def write_chunk_cv_sidecar(path: str, enc: int, rows_written: int, root: bytes, cvs: np.ndarray,
                           chunk_lo: int = 0, n_chunks: Optional[int] = None) -> None:
    """cvs = the CVs of chunks [chunk_lo, chunk_lo + len(cvs)); the other chunk rows of an existing
    sidecar stay.  The body is written first, then the header (a torn write leaves a header whose
    root no longer matches the tree, and the next attach rebuilds)."""
    cvs = np.ascontiguousarray(cvs, dtype=np.uint8).reshape(-1, enc, CV_BYTES)
    n_chunks = leaf_n_chunks(rows_written) if n_chunks is None else n_chunks
    if chunk_lo + cvs.shape[0] > n_chunks:
        raise ValueError("chunk rows beyond the sidecar")
    whole = chunk_lo == 0 and cvs.shape[0] == n_chunks
    if not whole and not os.path.isfile(path):
        raise FileNotFoundError("no chunk-CV sidecar to update")
    with open(path, "w+b" if whole else "r+b") as f:
        f.truncate(CHUNK_CV_HEADER_BYTES + n_chunks * enc * CV_BYTES)
        f.seek(CHUNK_CV_HEADER_BYTES + chunk_lo * enc * CV_BYTES)
        f.write(cvs.tobytes())
        f.flush()
        f.seek(0)
        f.write(encode_chunk_cv_header(enc, rows_written, n_chunks, root))


class ColumnChunkCache:
    """lcpc_pos_chunk_cache: every column's chunk CVs, resident on the GPU."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_porenc(cls, image: np.ndarray, enc: int, rows_written: int, row_capacity: int) -> "ColumnChunkCache":
        """One full pass over a `.porenc` image (a u8 array, typically over an mmap)."""
        h = N.vp()
        _raise(N.load().lcpc_pos_chunk_cache_from_porenc(_u8(image), enc, rows_written, row_capacity, C.byref(h)))
        return cls(h)

    @classmethod
    def from_cvs(cls, cvs, enc: int, rows_written: int) -> "ColumnChunkCache":
        a = np.ascontiguousarray(cvs, dtype=np.uint8).reshape(-1)
        if a.size != leaf_n_chunks(rows_written) * enc * CV_BYTES:
            raise ValueError("cvs must hold leaf_n_chunks(rows_written) * enc chaining values")
        h = N.vp()
        _raise(N.load().lcpc_pos_chunk_cache_from_cvs(_u8(a), enc, rows_written, C.byref(h)))
        return cls(h)

    @staticmethod
    def update_chunk_range(old_rows: int, new_rows: int, row_lo: int, row_hi: int) -> Tuple[int, int]:
        """The chunks [lo, hi) an update rehashes (lcpc_pos_update_chunk_range; host only)."""
        lo, hi = C.c_size_t(), C.c_size_t()
        _raise(N.load().lcpc_pos_update_chunk_range(old_rows, new_rows, row_lo, row_hi, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    @property
    def enc(self) -> int:
        return N.load().lcpc_pos_chunk_cache_enc(self._h)

    @property
    def rows(self) -> int:
        return N.load().lcpc_pos_chunk_cache_rows(self._h)

    @property
    def n_chunks(self) -> int:
        return N.load().lcpc_pos_chunk_cache_n_chunks(self._h)

    def copy_cvs(self, chunk_lo: int = 0, chunk_hi: Optional[int] = None) -> np.ndarray:
        chunk_hi = self.n_chunks if chunk_hi is None else chunk_hi
        out = np.zeros((max(chunk_hi - chunk_lo, 0), self.enc, CV_BYTES), np.uint8)
        _raise(N.load().lcpc_pos_chunk_cache_copy_cvs(self._h, chunk_lo, chunk_hi, _u8(out)))
        return out

    def update(self, image: np.ndarray, row_capacity: int, row_lo: int, row_hi: int,
               new_rows_written: int) -> Tuple[int, int]:
        """Rows [row_lo, row_hi) of the image changed, the file now has new_rows_written rows:
        rehash the affected chunks only; returns the chunk range rewritten."""
        lo, hi = C.c_size_t(), C.c_size_t()
        _raise(N.load().lcpc_pos_chunk_cache_update(self._h, _u8(image), row_capacity, row_lo, row_hi,
                                                    new_rows_written, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def update_file(self, encoded_file, row_capacity: int, row_lo: int, row_hi: int,
                    new_rows_written: int) -> Tuple[int, int]:
        """update() with the image read from the open `.porenc` file (pread of the affected
        slices): no mapping of the whole file for 1 KiB per column."""
        lo, hi = C.c_size_t(), C.c_size_t()
        _raise(N.load().lcpc_pos_chunk_cache_update_fd(self._h, encoded_file.fileno(), row_capacity, row_lo, row_hi,
                                                       new_rows_written, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def digests(self) -> np.ndarray:
        d = np.zeros((self.enc, DIGEST_BYTES), np.uint8)
        _raise(N.load().lcpc_pos_chunk_cache_tree(self._h, _u8(d), None))
        return d

    def tree(self) -> MerkleTree:
        t = np.zeros((2 * self.enc - 1, DIGEST_BYTES), np.uint8)
        _raise(N.load().lcpc_pos_chunk_cache_tree(self._h, None, _u8(t)))
        return MerkleTree(t)

    def close(self) -> None:
        if self._h is not None:
            N.load().lcpc_pos_chunk_cache_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- mapped file images
class _Image:
    """A read/write mmap of a `.porenc` file (zero-length files map to nothing)."""

    def __init__(self, f, size: int):
        self.f = f
        self.size = size
        f.truncate(size)
        f.flush()
        self.mm = mmap.mmap(f.fileno(), size) if size else None
        self.arr = np.frombuffer(self.mm, np.uint8) if size else np.zeros(0, np.uint8)

    def ptr(self):
        return _u8(self.arr)

    def close(self):
        if self.mm is not None:
            self.mm.flush()
            del self.arr
            self.mm.close()
            self.mm = None
            self.arr = np.zeros(0, np.uint8)

    def grow(self, old_rows: int, new_rows: int, n_cols: int) -> None:
        """EncodedFileReader::set_new_capacity (reader.rs:348-381): columns move back to
        front to their new stride, the space after each zeroed."""
        wb = WRITTEN_BYTES_WIDTH
        self.close()
        self.__init__(self.f, new_rows * n_cols * wb)
        a = self.arr
        old_len, new_len = old_rows * wb, new_rows * wb
        for c in range(n_cols - 1, 0, -1):
            a[c * new_len:c * new_len + old_len] = a[c * old_len:(c + 1) * old_len].copy()
            a[c * new_len + old_len:(c + 1) * new_len] = 0
        a[old_len:new_len] = 0


# ---------------------------------------------------------------- writer
class EncodedFileWriter:
    """EncodedFileWriter<WriteableFt63, Blake3, LigeroEncoding> (encoded_file_writer.rs)."""

    def __init__(self, num_pre_encoded_columns: int, num_encoded_columns: int,
                 original_file_size: int, target_file, batch_rows: int = 0):
        # new (:53-105): the assertions, then the file preallocated to 2 * rows
        if not (num_encoded_columns > 0 and num_encoded_columns & (num_encoded_columns - 1) == 0):
            raise ValueError("num_encoded_columns must be a power of two")
        if not num_pre_encoded_columns < num_encoded_columns:
            raise ValueError("num_pre_encoded_columns must be less than num_encoded_columns")
        if not num_pre_encoded_columns > 0:
            raise ValueError("num_pre_encoded_columns must be > 0")
        self.pre_encoded_size = num_pre_encoded_columns
        self.encoded_size = num_encoded_columns
        num_rows = -(-(-(-original_file_size // DATA_BYTE_CAPACITY)) // num_pre_encoded_columns)
        self.row_capacity = num_rows * 2
        self.bytes_received = 0
        self.rows_written = 0
        self._img = _Image(target_file, self.row_capacity * num_encoded_columns * WRITTEN_BYTES_WIDTH)
        h = N.vp()
        _raise(N.load().lcpc_pos_writer_new(num_pre_encoded_columns, num_encoded_columns,
                                            self._img.ptr(), self.row_capacity, batch_rows, C.byref(h)))
        self._h = h
        self._done = False

    def _rows_for(self, n_bytes: int) -> int:
        return -(-(-(-n_bytes // DATA_BYTE_CAPACITY)) // self.pre_encoded_size)

    def _ensure_capacity(self, rows: int) -> None:
        # the reference doubles the capacity whenever the rows written reach it (:378-381)
        new_cap = self.row_capacity
        while rows >= new_cap > 0:
            new_cap *= 2
        if rows > new_cap:  # zero-capacity files (empty original)
            new_cap = max(rows, 1) * 2
        if new_cap == self.row_capacity:
            return
        self._img.grow(self.row_capacity, new_cap, self.encoded_size)
        self.row_capacity = new_cap
        _raise(N.load().lcpc_pos_writer_set_target(self._h, self._img.ptr(), new_cap))

    def get_encoded_file_metadata(self) -> EncodedFileMetadata:
        return EncodedFileMetadata(self.pre_encoded_size, self.encoded_size, self.rows_written,
                                   self.row_capacity, self.bytes_received)

    def push_bytes(self, data: bytes) -> None:
        if self._done:
            raise RuntimeError("writer already finalized")
        self._ensure_capacity(self._rows_for(self.bytes_received + len(data)))
        p, keep = _bytes_ptr(data)
        _raise(N.load().lcpc_pos_writer_push_bytes(self._h, p, len(data)))
        self.bytes_received += len(data)

    def _finalize(self, want_digests: bool, want_tree: bool, keep_chunk_cvs: bool = False):
        if self._done:
            raise RuntimeError("writer already finalized")
        self._ensure_capacity(self._rows_for(self.bytes_received))
        w = self.encoded_size
        digests = np.zeros((w, DIGEST_BYTES), np.uint8) if want_digests else None
        tree = np.zeros((2 * w - 1, DIGEST_BYTES), np.uint8) if want_tree else None
        rows, nbytes = C.c_size_t(), C.c_size_t()
        try:
            _raise(N.load().lcpc_pos_writer_finalize(
                self._h, _u8(digests) if want_digests else None, _u8(tree) if want_tree else None,
                C.byref(rows), C.byref(nbytes)))
            if keep_chunk_cvs:  # the [chunk][column] CVs the digests were folded from
                self.chunk_cvs = _writer_chunk_cvs(self._h, w)
        finally:
            self._done = True
            N.load().lcpc_pos_writer_free(self._h)
            self._img.close()
        self.rows_written = rows.value
        return digests, tree

    def finalize_to_column_digest(self) -> Tuple[EncodedFileMetadata, List[bytes]]:
        d, _ = self._finalize(True, False)
        return self.get_encoded_file_metadata(), [r.tobytes() for r in d]

    def finalize_to_commit(self) -> Tuple[EncodedFileMetadata, bytes]:
        _, t = self._finalize(False, True)
        return self.get_encoded_file_metadata(), t[-1].tobytes()

    def finalize_to_merkle_tree(self, keep_chunk_cvs: bool = False) -> Tuple[EncodedFileMetadata, MerkleTree]:
        """keep_chunk_cvs: also leave the column chunk CVs in self.chunk_cvs (ColumnChunkCache)."""
        _, t = self._finalize(False, True, keep_chunk_cvs)
        return self.get_encoded_file_metadata(), MerkleTree(t)

    def __del__(self):
        if getattr(self, "_done", True) is False:
            try:
                N.load().lcpc_pos_writer_free(self._h)
                self._img.close()
            except Exception:
                pass

    @staticmethod
    def convert_unencoded_file(unencoded_file, target_encoded_file: str,
                               target_digest_file: Optional[str], target_metadata_file: Optional[str],
                               num_pre_encoded_columns: int, num_encoded_columns: int,
                               target_chunk_cv_file: Optional[str] = None
                               ) -> Tuple[EncodedFileMetadata, MerkleTree]:
        """encoded_file_writer.rs:134-231: the whole file in one pass of the GPU writer.
        target_chunk_cv_file: also write the `.porcv` sidecar, from the CVs that pass computed."""
        if num_pre_encoded_columns < 1:
            raise ValueError("Number of pre-encoded columns must be greater than 0")
        if num_encoded_columns < 2 or num_encoded_columns & (num_encoded_columns - 1):
            raise ValueError("Number of encoded columns must be a power of 2")
        if num_encoded_columns <= num_pre_encoded_columns:
            raise ValueError("Number of encoded columns must be greater than the number of columns")
        unencoded_file.seek(0, os.SEEK_END)
        total = unencoded_file.tell()
        unencoded_file.seek(0)
        num_rows = -(-(-(-total // DATA_BYTE_CAPACITY)) // num_pre_encoded_columns)
        cap = num_rows * 2
        with open(target_encoded_file, "w+b") as tf:
            img = _Image(tf, cap * num_encoded_columns * WRITTEN_BYTES_WIDTH)
            src = mmap.mmap(unencoded_file.fileno(), total, access=mmap.ACCESS_READ) if total else None
            try:
                data = np.frombuffer(src, np.uint8) if total else np.zeros(0, np.uint8)
                tree = np.zeros((2 * num_encoded_columns - 1, DIGEST_BYTES), np.uint8)
                rows = C.c_size_t()
                cvs = None
                if target_chunk_cv_file is None:
                    _raise(N.load().lcpc_pos_encode_file(_u8(data), total, num_pre_encoded_columns,
                                                         num_encoded_columns, cap, img.ptr(), _u8(tree),
                                                         C.byref(rows)))
                else:  # the same writer, called in steps so its CVs can be taken before it goes
                    h = N.vp()
                    _raise(N.load().lcpc_pos_writer_new(num_pre_encoded_columns, num_encoded_columns,
                                                        img.ptr(), cap, 0, C.byref(h)))
                    try:
                        _raise(N.load().lcpc_pos_writer_push_bytes(h, _u8(data), total))
                        _raise(N.load().lcpc_pos_writer_finalize(h, None, _u8(tree), C.byref(rows), None))
                        cvs = _writer_chunk_cvs(h, num_encoded_columns)
                    finally:
                        N.load().lcpc_pos_writer_free(h)
                del data
            finally:
                if src is not None:
                    src.close()
                img.close()
        meta = EncodedFileMetadata(num_pre_encoded_columns, num_encoded_columns, rows.value, cap, total)
        mt = MerkleTree(tree)
        if target_metadata_file:
            with open(target_metadata_file, "wb") as f:
                meta.write_to_file(f)
        if target_digest_file:
            with open(target_digest_file, "wb") as f:
                write_tree_to_file(f, mt)
        if target_chunk_cv_file:
            write_chunk_cv_sidecar(target_chunk_cv_file, num_encoded_columns, rows.value, mt.root(), cvs)
        return meta, mt

    @staticmethod
    def convert_unencoded_files(items) -> List[Tuple[EncodedFileMetadata, MerkleTree]]:
        """convert_unencoded_file for many files in one grouped pass (lcpc_pos_encode_files_grouped): items
        is a sequence of its argument tuples (unencoded_file, target_encoded_file, target_digest_file,
        target_metadata_file, num_pre_encoded_columns, num_encoded_columns[, target_chunk_cv_file]).  Every
        file written is byte for byte what the single call writes; the launches do not grow with the
        number of files.  Every item's dims are checked before the first target is created."""
        from .pos import encode_files_grouped_into
        items = [tuple(it) + (None,) * (7 - len(it)) for it in items]
        for it in items:
            pre, enc = it[4], it[5]
            if pre < 1:
                raise ValueError("Number of pre-encoded columns must be greater than 0")
            if enc < 2 or enc & (enc - 1):
                raise ValueError("Number of encoded columns must be a power of 2")
            if enc <= pre:
                raise ValueError("Number of encoded columns must be greater than the number of columns")
        if not items:
            return []
        totals, caps, files, imgs, srcs, datas = [], [], [], [], [], []
        try:
            for src_f, target, _, _, pre, enc, _ in items:
                src_f.seek(0, os.SEEK_END)
                total = src_f.tell()
                src_f.seek(0)
                cap = 2 * (-(-(-(-total // DATA_BYTE_CAPACITY)) // pre))
                tf = open(target, "w+b")
                files.append(tf)
                imgs.append(_Image(tf, cap * enc * WRITTEN_BYTES_WIDTH))
                src = mmap.mmap(src_f.fileno(), total, access=mmap.ACCESS_READ) if total else None
                srcs.append(src)
                datas.append(np.frombuffer(src, np.uint8) if total else np.zeros(0, np.uint8))
                totals.append(total)
                caps.append(cap)
            res = encode_files_grouped_into(datas, [it[4] for it in items], [it[5] for it in items],
                                            [im.arr for im in imgs], caps, True, False,
                                            [it[6] is not None for it in items])
        finally:
            del datas
            for src in srcs:
                if src is not None:
                    src.close()
            for im in imgs:
                im.close()
            for tf in files:
                tf.close()
        out = []
        for it, total, cap, o in zip(items, totals, caps, res):
            _, _, digest_file, meta_file, pre, enc, cv_file = it
            meta = EncodedFileMetadata(pre, enc, o["rows_written"], cap, total)
            mt = MerkleTree(o["tree"])
            if meta_file:
                with open(meta_file, "wb") as f:
                    meta.write_to_file(f)
            if digest_file:
                with open(digest_file, "wb") as f:
                    write_tree_to_file(f, mt)
            if cv_file:
                write_chunk_cv_sidecar(cv_file, enc, o["rows_written"], mt.root(), o["cvs"])
            out.append((meta, mt))
        return out


def _writer_chunk_cvs(writer_handle, enc: int) -> np.ndarray:
    """The [chunk][column] CVs of a finalized lcpc_pos_writer."""
    n = N.load().lcpc_pos_writer_n_chunks(writer_handle)
    cvs = np.zeros((n, enc, CV_BYTES), np.uint8)
    _raise(N.load().lcpc_pos_writer_copy_cvs(writer_handle, _u8(cvs)))
    return cvs


# ---------------------------------------------------------------- streamed rows
class ColumnsToCareAbout:
    """column_digest_accumulator.rs:9-15.  Only(indices) is kept as a type; the accumulator
    refuses it (see ColumnDigestAccumulator)."""
    All = "All"

    @dataclass
    class Only:
        indices: List[int]


class ColumnDigestAccumulator:
    """ColumnDigestAccumulator<Blake3, F> (column_digest_accumulator.rs:17-118) over the GPU
    accumulator (lcpc_column_digests_*): every column's digest is BLAKE3(32 zero bytes || repr of
    its elements), hashed in 1-KiB chunks as they complete, so memory stays one batch of rows.
    update takes one encoded row (num_encoded elements) or a (k, num_encoded) batch of them.

    ColumnsToCareAbout.Only raises NotImplementedError: the reference's update checks the row
    length against the number of tracked columns and then indexes the digests by column number
    (:63-84), so it only works where it equals All; no caller uses it."""

    def __init__(self, number_of_encoded_columns: int, columns_to_care_about=ColumnsToCareAbout.All,
                 field: int = 0, batch_rows: int = 0):
        if isinstance(columns_to_care_about, ColumnsToCareAbout.Only):
            raise NotImplementedError("ColumnsToCareAbout::Only (unusable in the reference; see the class doc)")
        self.field = field
        self._nl = L.limbs(field)
        h = N.vp()
        _raise(N.load().lcpc_column_digests_new(field, number_of_encoded_columns, batch_rows, C.byref(h)))
        self._h = h
        self._done = False

    def get_width(self) -> int:
        return N.load().lcpc_column_digests_width(self._h)

    def update(self, encoded_row) -> None:
        if self._done:
            raise RuntimeError("accumulator already finalized")
        a = np.ascontiguousarray(encoded_row, dtype=np.uint64)
        w = self.get_width()
        if a.size % (w * self._nl):
            raise ValueError("incorrect length of input")  # ensure! (:63-66)
        n = a.size // (w * self._nl)
        _raise(N.load().lcpc_column_digests_update(self._h, L._p64(a.reshape(-1)) if n else None, n))

    def _finalize(self, want_digests: bool, want_tree: bool):
        if self._done:
            raise RuntimeError("accumulator already finalized")
        w = self.get_width()
        digests = np.zeros((w, DIGEST_BYTES), np.uint8) if want_digests else None
        tree = np.zeros((2 * w - 1, DIGEST_BYTES), np.uint8) if want_tree else None
        try:
            _raise(N.load().lcpc_column_digests_finalize(self._h, _u8(digests) if want_digests else None,
                                                         _u8(tree) if want_tree else None))
        finally:
            self._done = True
            N.load().lcpc_column_digests_free(self._h)
        return digests, tree

    def get_column_digests(self) -> List[bytes]:
        d, _ = self._finalize(True, False)
        return [r.tobytes() for r in d]

    def finalize_to_commit(self) -> bytes:
        return self.finalize_to_merkle_tree().root()

    def finalize_to_merkle_tree(self) -> MerkleTree:
        _, t = self._finalize(False, True)
        return MerkleTree(t)

    def __del__(self):
        if getattr(self, "_done", True) is False:
            try:
                N.load().lcpc_column_digests_free(self._h)
            except Exception:
                pass


class RowGeneratorIter:
    """RowGeneratorIter<WriteableFt63, I, LigeroEncoding> (row_generator_iter.rs:8-165).

    Iterating yields the encoded rows (num_encoded elements each, uint64 raw limbs): every
    num_pre_encoded elements of `field_iterator` (the last row zero padded) Ligero-encoded, as
    `next` (:138-164) does row by row.  Here up to `batch_rows` rows are taken from the iterator at
    once and encoded in one GPU call (lcpc_encode_rows), then handed out one by one.

    The consuming methods work on the rows not yet yielded:
      get_column_digests / get_specified_column_digests / convert_to_commit_root (:29-77) stream
        them through a digest-only PoS writer (lcpc_pos_writer_new with no image), so memory stays
        one batch however long the input;
      get_full_columns (:79-107) commits to them and opens the columns.  Like the reference, it
        returns the columns in REVERSE order of `specified_columns` (it pops the last first,
        :99-104).
    From a FieldGeneratorIter (whole 7-byte data words) the data bytes go straight to the
    writer.  Any other element iterator streams its encoded rows through a
    ColumnDigestAccumulator, as the reference does (:33-40)."""

    def __init__(self, field_iterator, num_pre_encoded: int, num_encoded: int, batch_rows: int = 1024):
        if not (num_encoded > 0 and num_encoded & (num_encoded - 1) == 0) or not 0 < num_pre_encoded < num_encoded:
            raise ValueError("bad Ligero dimensions")
        self.field_iterator = field_iterator
        self.unencoded_len = num_pre_encoded
        self.encoded_len = num_encoded
        self.encoding = L.LigeroEncoding.new_from_dims(L.FT63, num_pre_encoded, num_encoded)
        self.batch_rows = max(1, batch_rows)
        self._elems = np.zeros(0, np.uint64)   # unencoded elements of the rows in _rows
        self._rows = np.zeros((0, num_encoded), np.uint64)
        self._next = 0

    @classmethod
    def new_ligero(cls, field_iterator, num_pre_encoded: int, num_encoded: int) -> "RowGeneratorIter":
        return cls(field_iterator, num_pre_encoded, num_encoded)

    def _take(self, n: int) -> np.ndarray:
        return np.fromiter(itertools.islice(self.field_iterator, n), dtype=np.uint64)

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        if self._next == self._rows.shape[0]:
            pre, enc = self.unencoded_len, self.encoded_len
            el = self._take(self.batch_rows * pre)
            if el.size == 0:  # the empty case (:148-151)
                raise StopIteration
            n = -(-el.size // pre)
            flat = np.zeros(n * pre, np.uint64)
            flat[:el.size] = el
            m = np.zeros((n, enc), np.uint64)
            m[:, :pre] = flat.reshape(n, pre)
            self._rows = self.encoding.encode_rows(m).reshape(n, enc)
            self._elems = el
            self._next = 0
        row = self._rows[self._next].copy()
        self._next += 1
        return row

    def _rest_elements(self) -> np.ndarray:
        """The unencoded elements of every row not yet yielded (consumes the iterator)."""
        pre = self.unencoded_len
        head = self._elems[self._next * pre:]
        self._rows, self._elems, self._next = self._rows[:0], self._elems[:0], 0
        tail = np.fromiter(self.field_iterator, dtype=np.uint64)
        return np.concatenate([head, tail])

    def _rest_byte_blocks(self):
        """The rows not yet yielded as data bytes (FieldGeneratorIter inputs only)."""
        pre = self.unencoded_len
        head = self._elems[self._next * pre:]
        self._rows, self._elems, self._next = self._rows[:0], self._elems[:0], 0
        if head.size:
            yield head.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :DATA_BYTE_CAPACITY].tobytes()
        yield from self.field_iterator.byte_blocks()

    def _digests_and_tree(self):
        from .pos import FieldGeneratorIter
        w = self.encoded_len
        digests = np.zeros((w, DIGEST_BYTES), np.uint8)
        tree = np.zeros((2 * w - 1, DIGEST_BYTES), np.uint8)
        if not isinstance(self.field_iterator, FieldGeneratorIter):
            acc = ColumnDigestAccumulator(w, ColumnsToCareAbout.All, L.FT63)
            batch = []
            for row in self:
                batch.append(row)
                if len(batch) == self.batch_rows:
                    acc.update(np.stack(batch))
                    batch = []
            if batch:
                acc.update(np.stack(batch))
            tree = acc.finalize_to_merkle_tree()
            return tree.digests[:w].copy(), tree.digests.copy()
        h = N.vp()
        _raise(N.load().lcpc_pos_writer_new(self.unencoded_len, w, None, 0, 0, C.byref(h)))
        try:
            for block in self._rest_byte_blocks():
                p, keep = _bytes_ptr(block)
                _raise(N.load().lcpc_pos_writer_push_bytes(h, p, len(block)))
            rows, nbytes = C.c_size_t(), C.c_size_t()
            _raise(N.load().lcpc_pos_writer_finalize(h, _u8(digests), _u8(tree), C.byref(rows), C.byref(nbytes)))
        finally:
            N.load().lcpc_pos_writer_free(h)
        return digests, tree

    def get_column_digests(self) -> List[bytes]:
        d, _ = self._digests_and_tree()
        return [r.tobytes() for r in d]

    def get_specified_column_digests(self, column_indices) -> List[bytes]:
        d = self.get_column_digests()
        return [d[i] for i in column_indices]

    def convert_to_commit_root(self) -> bytes:
        _, t = self._digests_and_tree()
        return t[-1].tobytes()

    def get_full_columns(self, specified_columns) -> List["L.LcColumn"]:
        el = self._rest_elements()
        comm = L.LcCommit.commit(el.reshape(-1, 1), self.encoding)
        return comm.open_columns(list(specified_columns))[::-1]


# ---------------------------------------------------------------- reader
class EncodedFileReader:
    """EncodedFileReader<WriteableFt63, Blake3, LigeroEncoding> (encoded_file_reader.rs)."""

    def __init__(self, file_to_read, pre_encoded_size: int, encoded_size: int, rows_written: int,
                 row_capacity: int):
        self.f = file_to_read
        self.pre_encoded_size = pre_encoded_size
        self.encoded_size = encoded_size
        self.rows_written = rows_written
        self.row_capacity = row_capacity

    @classmethod
    def new_ligero(cls, file_to_read, pre_encoded_size, encoded_size, rows_written, row_capacity):
        return cls(file_to_read, pre_encoded_size, encoded_size, rows_written, row_capacity)

    def _with_map(self, fn):
        """fn(u8 array over a read-only mmap of the file); no view of it may escape fn."""
        size = os.fstat(self.f.fileno()).st_size
        need = self.row_capacity * self.encoded_size * WRITTEN_BYTES_WIDTH
        if size < need:
            raise ValueError("encoded file shorter than row_capacity * encoded_size elements")
        if need == 0:
            return fn(np.zeros(0, np.uint8))
        mm = mmap.mmap(self.f.fileno(), need, access=mmap.ACCESS_READ)
        try:
            return fn(np.frombuffer(mm, np.uint8))
        finally:
            try:
                mm.close()
            except BufferError:  # an in-flight exception's traceback still holds the view
                pass

    def get_encoded_column_without_path(self, target_col: int) -> np.ndarray:
        """Canonical u64 values of the column's rows_written elements (reader.rs:317-326)."""
        wb = WRITTEN_BYTES_WIDTH
        self.f.seek(target_col * self.row_capacity * wb)
        raw = self.f.read(self.rows_written * wb)
        return np.frombuffer(raw, "<u8").copy()

    def get_encoded_row(self, target_row: int) -> np.ndarray:
        """Canonical u64 values of the row's encoded_size elements (reader.rs:214-253)."""
        return self._with_map(lambda a: a.view("<u8").reshape(self.encoded_size, self.row_capacity)
                              [:, target_row].copy())

    def get_unencoded_row_bytes(self, target_row: int) -> bytes:
        if not target_row < self.rows_written:
            raise IndexError("target row index is out of bounds")
        return self._decode(target_row, target_row + 1)

    def _decode(self, lo: int, hi: int) -> bytes:
        out = np.zeros((hi - lo) * self.pre_encoded_size * DATA_BYTE_CAPACITY, np.uint8)
        self._with_map(lambda a: _raise(N.load().lcpc_pos_decode_porenc(
            _u8(a), self.pre_encoded_size, self.encoded_size, self.row_capacity, lo, hi, _u8(out))))
        return out.tobytes()

    def get_unencoded_row(self, target_row: int) -> np.ndarray:
        """The row's pre_encoded_size elements, raw limbs (WriteableFt63 internal words)."""
        b = self.get_unencoded_row_bytes(target_row)
        return np.frombuffer(b"".join(b[i:i + 7] + b"\0" for i in range(0, len(b), 7)), "<u8").copy()

    def decode_to_target_file(self, target_file) -> None:
        """reader.rs:79-91: every written row's pre_encoded_size * 7 bytes, in order."""
        if self.rows_written:
            target_file.write(self._decode(0, self.rows_written))
        target_file.flush()

    def get_unencoded_file_len(self) -> int:
        return os.fstat(self.f.fileno()).st_size // (self.encoded_size // self.pre_encoded_size)

    def process_file_to_merkle_tree(self) -> MerkleTree:
        w = self.encoded_size
        tree = np.zeros((2 * w - 1, DIGEST_BYTES), np.uint8)
        self._with_map(lambda a: _raise(N.load().lcpc_pos_porenc_tree(
            _u8(a), w, self.rows_written, self.row_capacity, _u8(tree))))
        return MerkleTree(tree)

    # -- scrub and repair (no counterpart in the reference: include/lcpc_mi.h, "R-S erasure decoding")
    def _scrub(self, leaves: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(status, digests): status[c] = 0 the column's digest equals leaves[c], 1 it differs, 2 the
        column holds a non-canonical element (its digest is then zeros)."""
        w = self.encoded_size
        lv = np.ascontiguousarray(leaves, dtype=np.uint8).reshape(-1)
        if lv.size != w * DIGEST_BYTES:
            raise ValueError("one 32-byte leaf per encoded column is needed")
        status = np.zeros(w, np.uint8)
        digests = np.zeros((w, DIGEST_BYTES), np.uint8)
        n_bad = C.c_size_t()
        self._with_map(lambda a: _raise(N.load().lcpc_pos_scrub_porenc(
            _u8(a), w, self.rows_written, self.row_capacity, _u8(lv), _u8(digests), _u8(status), C.byref(n_bad))))
        return status, digests

    def find_damaged_columns(self, tree: MerkleTree) -> Tuple[List[int], List[int]]:
        """(bad, noncanonical): the columns whose digest differs from their leaf of `tree` (those
        that hold a non-canonical element included), and the non-canonical ones among them.  Rows
        past rows_written are not looked at."""
        status, _ = self._scrub(tree.digests[:self.encoded_size])
        return [int(c) for c in np.flatnonzero(status)], [int(c) for c in np.flatnonzero(status == 2)]

    def _locate(self, known_bad=()) -> Tuple[np.ndarray, int, int]:
        """(col_status, dirty_rows, unlocatable_rows) of lcpc_pos_locate_porenc."""
        w = self.encoded_size
        known = np.ascontiguousarray(np.asarray(list(known_bad), dtype=np.uint64).reshape(-1))
        status = np.zeros(w, np.uint8)
        n_bad, n_dirty, n_unloc = C.c_size_t(), C.c_size_t(), C.c_size_t()

        def run(a):
            code = N.load().lcpc_pos_locate_porenc(
                _u8(a), self.pre_encoded_size, w, self.rows_written, self.row_capacity,
                known.ctypes.data_as(N.u64p) if known.size else None, known.size, _u8(status),
                C.byref(n_bad), C.byref(n_dirty), C.byref(n_unloc))
            if code == LCPC_ERR_UNRECOVERABLE:
                raise UnrecoverableError(N.last_error())
            _raise(code)
        self._with_map(run)
        return status, int(n_dirty.value), int(n_unloc.value)

    def locate_damaged_columns(self, known_bad=()) -> Tuple[np.ndarray, int]:
        """The damaged columns by the code's own redundancy, without a tree: every row's syndromes,
        Berlekamp-Massey and a root search name the wrong elements of up to
        (encoded_size - pre_encoded_size - erasures) // 2 columns per row.  Returns (col_status,
        unlocatable_rows): col_status[c] = 0 nothing found, 1 a wrong element was located in some
        row, 2 the column holds an element that is not < p, 3 listed in known_bad (never read).
        unlocatable_rows > 0: some rows hold more wrong elements than can be located, and their
        columns are not named.  UnrecoverableError if the known and the non-canonical columns
        outnumber the code's redundancy."""
        status, _, n_unloc = self._locate(known_bad)
        return status, n_unloc

    def _repair(self, columns, want_cols: bool, want_digests: bool, want_data: bool):
        cols_idx = np.ascontiguousarray(np.asarray(list(columns), dtype=np.uint64).reshape(-1))
        k, rows = cols_idx.size, self.rows_written
        cols = np.zeros((k, rows), "<u8") if want_cols else None
        digests = np.zeros((k, DIGEST_BYTES), np.uint8) if want_digests else None
        data = np.zeros(rows * self.pre_encoded_size * DATA_BYTE_CAPACITY, np.uint8) if want_data else None

        def ptr(a):
            return a.ctypes.data_as(N.u8p) if a is not None and a.size else None

        def run(a):
            code = N.load().lcpc_pos_repair_columns(
                _u8(a), self.pre_encoded_size, self.encoded_size, rows, self.row_capacity,
                cols_idx.ctypes.data_as(N.u64p) if k else None, k, ptr(cols), ptr(digests), ptr(data))
            if code == LCPC_ERR_UNRECOVERABLE:
                raise UnrecoverableError(N.last_error())
            _raise(code)
        self._with_map(run)
        return cols, digests, data

    def repair_columns(self, columns) -> Tuple[np.ndarray, np.ndarray]:
        """The listed columns recomputed from all the others (which alone are read): (cols, digests),
        cols[k] = the rows_written canonical u64 values of column columns[k] as they belong in the
        file, digests[k] its 32-byte column digest.  At most encoded_size - pre_encoded_size columns;
        UnrecoverableError beyond that, or when the other columns do not form codewords.  The file
        is not written."""
        cols, digests, _ = self._repair(columns, True, True, False)
        return cols, digests

    def decode_with_erasures(self, columns) -> bytes:
        """decode_to_target_file's bytes (rows_written * pre_encoded_size * 7) without reading the
        listed columns: the recovery path for a download from a damaged replica."""
        return self._repair(columns, False, False, True)[2].tobytes()

    def set_new_capacity(self, new_row_capacity: int) -> None:
        if new_row_capacity < self.rows_written:
            raise ValueError("Cannot set capacity to fewer than rows are written.")
        img = _Image.__new__(_Image)
        img.f, img.size = self.f, self.row_capacity * self.encoded_size * WRITTEN_BYTES_WIDTH
        img.mm = None
        img.arr = np.zeros(0, np.uint8)
        img.grow(self.row_capacity, new_row_capacity, self.encoded_size)
        img.close()
        self.row_capacity = new_row_capacity

    def resize_to_target_file(self, target_file, new_pre_encoded_size: int, new_encoded_size: int
                              ) -> Tuple[EncodedFileMetadata, MerkleTree]:
        """reader.rs:98-117: decode every row, push its bytes into a writer of the new shape."""
        w = EncodedFileWriter(new_pre_encoded_size, new_encoded_size, self.get_unencoded_file_len(),
                              target_file)
        if self.rows_written:
            w.push_bytes(self._decode(0, self.rows_written))
        return w.finalize_to_merkle_tree()


# ---------------------------------------------------------------- file handler
SERVER_FILE_FOLDER = "PoR_server_files"   # databases/constants.rs:1-5
UNENCODED_FILE_EXTENSION, ENCODED_FILE_EXTENSION = "porraw", "porenc"
MERKLE_FILE_EXTENSION, METADATA_FILE_EXTENSION = "portree", "meta"


def _location(directory: Optional[str], ulid: str, ext: str) -> str:
    """file_formatter.rs get_*_file_location_from_id: <dir>/<ulid>.<ext>, dir created on demand
    (the reference's dir is <cwd>/PoR_server_files)."""
    d = directory if directory is not None else os.path.join(os.getcwd(), SERVER_FILE_FOLDER)
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, f"{ulid}.{ext}")


class FileHandler:
    """FileHandler<Blake3, WriteableFt63, LigeroEncoding> (lcpc_online/file_handler.rs:29-712).

    The server-side owner of one stored file: the raw `.porraw` bytes, the column-major
    `.porenc` codeword, the `.portree` Merkle tree and the `.meta` JSON.  Edits and appends
    re-encode only the touched rows (lcpc_pos_reencode_rows: pack, NTT and transpose on the GPU,
    written into the mapped `.porenc`), then rebuild the tree from the file on the GPU
    (lcpc_pos_porenc_tree), as the reference's edit_bytes / append_bytes do.

    chunk_cache=True (off by default; nothing changes without it) keeps a ColumnChunkCache and its
    `<ulid>.porcv` sidecar next to the four files: edit_bytes and append_bytes then reread and
    rehash only the 1-KiB column chunks they touched and fold the tree from the cache, instead of
    the whole `.porenc`.  The `.porenc`, `.portree` and `.meta` files are the same either way.
    """

    def __init__(self, ulid: str, unencoded: str, encoded: str, merkle: str, metadata: str,
                 chunk_cache: bool = False):
        # new_attach_to_existing_files (:73-143)
        with open(metadata, "rb") as f:
            m = EncodedFileMetadata.read_from_file(f)
        if m.ulid != ulid:
            raise ValueError("supplied metadata file ulid does not match!")
        self.file_ulid = ulid
        self.pre_encoded_size, self.encoded_size = m.pre_encoded_size, m.encoded_size
        self.rows_written, self.row_capacity = m.rows_written, m.row_capacity
        self.total_data_bytes = m.bytes_of_data
        self.unencoded_file_handle, self.encoded_file_handle = unencoded, encoded
        self.merkle_tree_file_handle, self.metadata_file_handle = merkle, metadata
        with open(merkle, "rb") as f:
            self.merkle_tree = MerkleTree.from_bytes(f.read())
        self.chunk_cache: Optional[ColumnChunkCache] = None
        self.chunk_cv_file_handle = os.path.join(os.path.dirname(encoded), f"{ulid}.{CHUNK_CV_EXTENSION}")
        self.last_chunk_range = (0, 0)   # chunks the last edit / append rehashed (chunk_cache only)
        if chunk_cache:
            self._attach_chunk_cache()

    # -- construction
    @classmethod
    def new_attach_to_existing_ulid(cls, file_directory: str, ulid: str, chunk_cache: bool = False) -> "FileHandler":
        paths = [os.path.join(file_directory, f"{ulid}.{e}") for e in
                 (UNENCODED_FILE_EXTENSION, ENCODED_FILE_EXTENSION, MERKLE_FILE_EXTENSION, METADATA_FILE_EXTENSION)]
        for p, what in zip(paths, ("unencoded", "encoded", "merkle", "metadata")):
            if not os.path.isfile(p):
                raise FileNotFoundError(f"no {what} file found!")
        return cls(ulid, *paths, chunk_cache=chunk_cache)

    @classmethod
    def new_attach_to_existing_files(cls, ulid, unencoded, encoded, merkle, metadata,
                                     chunk_cache: bool = False) -> "FileHandler":
        return cls(ulid, unencoded, encoded, merkle, metadata, chunk_cache=chunk_cache)

    # -- the column chunk-CV cache (chunk_cache=True)
    def _with_image(self, fn):
        """fn(u8 array over a read-only mmap of the .porenc image); no view of it may escape fn."""
        with open(self.encoded_file_handle, "rb") as f:
            return self._reader(f)._with_map(fn)

    def _rebuild_chunk_cache(self) -> ColumnChunkCache:
        """One full pass over the .porenc (the cost of recalculate_merkle_tree)."""
        return self._with_image(lambda a: ColumnChunkCache.from_porenc(a, self.encoded_size, self.rows_written,
                                                                       self.row_capacity))

    def _attach_chunk_cache(self) -> None:
        """Load the sidecar if it belongs to this file as it stands (header against the metadata,
        length, root against the stored tree, and the CVs really fold to that root); otherwise --
        a missing sidecar included -- rebuild it from the .porenc and rewrite it."""
        cache = None
        try:
            with open(self.chunk_cv_file_handle, "rb") as f:
                header = f.read(CHUNK_CV_HEADER_BYTES)
                n_chunks = check_chunk_cv_sidecar(header, os.fstat(f.fileno()).st_size, self.encoded_size,
                                                  self.rows_written, self.merkle_tree.root())
                body = np.fromfile(f, np.uint8, n_chunks * self.encoded_size * CV_BYTES)
            cache = ColumnChunkCache.from_cvs(body, self.encoded_size, self.rows_written)
            if cache.tree() != self.merkle_tree:
                cache.close()
                cache = None
        except (OSError, ValueError):
            cache = None
        if cache is None:
            cache = self._rebuild_chunk_cache()
            write_chunk_cv_sidecar(self.chunk_cv_file_handle, self.encoded_size, self.rows_written,
                                   cache.tree().root(), cache.copy_cvs())
        if self.chunk_cache is not None:
            self.chunk_cache.close()
        self.chunk_cache = cache

    def _update_chunk_cache(self, row_lo: int, row_hi: int) -> MerkleTree:
        """After rows [row_lo, row_hi) were re-encoded into the .porenc (self.rows_written is the
        new count): rehash their chunks, fold the tree, rewrite those chunk rows of the sidecar
        and the .portree."""
        cache = self.chunk_cache
        with open(self.encoded_file_handle, "rb") as f:
            lo, hi = cache.update_file(f, self.row_capacity, row_lo, row_hi, self.rows_written)
        self.last_chunk_range = (lo, hi)
        tree = cache.tree()
        write_chunk_cv_sidecar(self.chunk_cv_file_handle, self.encoded_size, self.rows_written, tree.root(),
                               cache.copy_cvs(lo, hi), lo, cache.n_chunks)
        self.merkle_tree = tree
        self.write_tree(tree)
        return tree

    @classmethod
    def create_from_unencoded_file(cls, ulid: str, file_handle_if_not_already_ulid: Optional[str],
                                   pre_encoded_size: int, encoded_size: int,
                                   directory: Optional[str] = None, chunk_cache: bool = False) -> "FileHandler":
        """:145-199 -- the raw file is moved to <ulid>.porraw, then encoded (GPU writer)."""
        if encoded_size <= 0 or encoded_size & (encoded_size - 1):
            raise ValueError("encoded file size must be a power of two!")
        raw = _location(directory, ulid, UNENCODED_FILE_EXTENSION)
        enc = _location(directory, ulid, ENCODED_FILE_EXTENSION)
        tree = _location(directory, ulid, MERKLE_FILE_EXTENSION)
        meta = _location(directory, ulid, METADATA_FILE_EXTENSION)
        if file_handle_if_not_already_ulid is not None:
            os.rename(file_handle_if_not_already_ulid, raw)
        cv = _location(directory, ulid, CHUNK_CV_EXTENSION) if chunk_cache else None
        with open(raw, "r+b") as f:
            m, _ = EncodedFileWriter.convert_unencoded_file(f, enc, tree, meta, pre_encoded_size, encoded_size, cv)
        m.ulid = ulid
        with open(meta, "wb") as f:
            m.write_to_file(f)
        return cls(ulid, raw, enc, tree, meta, chunk_cache=chunk_cache)

    @classmethod
    def create_from_unencoded_files(cls, specs, directory: Optional[str] = None,
                                    chunk_cache: bool = False) -> List["FileHandler"]:
        """create_from_unencoded_file for many files in one grouped pass: specs is a sequence of (ulid,
        file_handle_if_not_already_ulid or None, pre_encoded_size, encoded_size).  The `.porraw`, `.porenc`,
        `.portree`, `.meta` and (chunk_cache) `.porcv` files are byte for byte those of a loop of the single
        call.  Every spec is checked before the first file is renamed or created."""
        specs = [tuple(s) for s in specs]
        for ulid, src, pre, enc in specs:
            if enc <= 0 or enc & (enc - 1):
                raise ValueError("encoded file size must be a power of two!")
            if pre < 1:
                raise ValueError("Number of pre-encoded columns must be greater than 0")
            if enc < 2 or enc <= pre:
                raise ValueError("Number of encoded columns must be greater than the number of columns")
            if src is not None and not os.path.isfile(src):
                raise FileNotFoundError(f"no unencoded file found for {ulid}!")
        if len({s[0] for s in specs}) != len(specs):
            raise ValueError("every file needs a ulid of its own")
        paths = []
        for ulid, src, pre, enc in specs:
            p = [_location(directory, ulid, e) for e in (UNENCODED_FILE_EXTENSION, ENCODED_FILE_EXTENSION,
                                                         MERKLE_FILE_EXTENSION, METADATA_FILE_EXTENSION)]
            p.append(_location(directory, ulid, CHUNK_CV_EXTENSION) if chunk_cache else None)
            if src is None and not os.path.isfile(p[0]):
                raise FileNotFoundError(f"no unencoded file found for {ulid}!")
            paths.append(p)
        for (ulid, src, pre, enc), p in zip(specs, paths):
            if src is not None:
                os.rename(src, p[0])
        raws = [open(p[0], "r+b") for p in paths]
        try:
            metas = EncodedFileWriter.convert_unencoded_files(
                [(f, p[1], p[2], p[3], pre, enc, p[4]) for f, p, (_, _, pre, enc) in zip(raws, paths, specs)])
        finally:
            for f in raws:
                f.close()
        out = []
        for (ulid, _, _, _), p, (m, _) in zip(specs, paths, metas):
            m.ulid = ulid
            with open(p[3], "wb") as f:
                m.write_to_file(f)
            out.append(cls(ulid, p[0], p[1], p[2], p[3], chunk_cache=chunk_cache))
        return out

    # -- accessors
    def get_encoded_file_handle(self) -> str:
        return self.encoded_file_handle

    def get_raw_file_handle(self) -> str:
        return self.unencoded_file_handle

    def get_merkle_file_handle(self) -> str:
        return self.merkle_tree_file_handle

    def get_dimensions(self) -> Tuple[int, int, int]:
        return self.pre_encoded_size, self.encoded_size, self.rows_written

    def get_encoded_metadata(self) -> EncodedFileMetadata:
        return EncodedFileMetadata(self.pre_encoded_size, self.encoded_size, self.rows_written,
                                   self.row_capacity, self.total_data_bytes, self.file_ulid)

    def get_total_data_bytes(self) -> int:
        return self.total_data_bytes

    get_total_unencoded_bytes = get_total_data_bytes

    def get_merkle_tree(self) -> MerkleTree:
        return self.merkle_tree

    def get_commit_root(self) -> bytes:
        """LcRoot::new_from_root_digest(tree.root()) (:648-651)."""
        return self.merkle_tree.root()

    def _reader(self, f) -> EncodedFileReader:
        return EncodedFileReader.new_ligero(f, self.pre_encoded_size, self.encoded_size, self.rows_written,
                                            self.row_capacity)

    def _row_bytes(self) -> int:
        return self.pre_encoded_size * DATA_BYTE_CAPACITY

    # -- raw data
    def left_multiply_unencoded_matrix_by_vector(self, left_vector) -> np.ndarray:
        """file_handler.rs:614-638: u^T M over the stored file's unencoded rows (left_vector has
        rows_written elements).  The reference's result vector is never sized, so it returns an
        empty vector; this returns the sum it is written to accumulate (pos.py's function)."""
        from .pos import left_multiply_unencoded_matrix_by_vector
        left = np.asarray(left_vector, dtype=np.uint64).reshape(-1)
        if left.size != self.rows_written:
            raise ValueError(f"left_vector incorrect size, expected {self.rows_written} and received {left.size}")
        with open(self.unencoded_file_handle, "rb") as f:
            data = f.read(self.total_data_bytes)
        return left_multiply_unencoded_matrix_by_vector(data, self.pre_encoded_size, left)

    def get_unencoded_bytes(self, byte_start: int, byte_end: int) -> bytes:
        with open(self.unencoded_file_handle, "rb") as f:
            f.seek(byte_start)
            b = f.read(byte_end - byte_start)
        if len(b) != byte_end - byte_start:
            raise EOFError("failed to fill whole buffer")
        return b

    def get_unencoded_row(self, row_index: int) -> bytes:
        """:585-602"""
        if not row_index < self.rows_written:
            raise IndexError("row_index out of bounds")
        rb = self._row_bytes()
        return self.get_unencoded_bytes(row_index * rb, min((row_index + 1) * rb, self.total_data_bytes))

    # -- encoded data
    def get_encoded_row(self, row_index: int) -> np.ndarray:
        with open(self.encoded_file_handle, "rb") as f:
            return self._reader(f).get_encoded_row(row_index)

    def get_decoded_row(self, row_index: int) -> np.ndarray:
        """:368-373 (decode_row of the encoded row, first pre_encoded_size elements)."""
        with open(self.encoded_file_handle, "rb") as f:
            return self._reader(f).get_unencoded_row(row_index)

    def get_decoded_row_bytes(self, row_index: int) -> bytes:
        with open(self.encoded_file_handle, "rb") as f:
            return self._reader(f).get_unencoded_row_bytes(row_index)

    def read_only_digests(self, columns=None) -> List[bytes]:
        """:550-564 (columns None = ColumnsToCareAbout::All)."""
        cols = range(self.encoded_size) if columns is None else columns
        return [self.merkle_tree[c] for c in cols]

    def read_full_columns(self, columns=None):
        """:566-583: LcColumn(col = the column's canonical values, path = its Merkle path)."""
        from .lcpc2d import LcColumn
        cols = range(self.encoded_size) if columns is None else columns
        with open(self.encoded_file_handle, "rb") as f:
            r = self._reader(f)
            out = []
            for c in cols:
                if not 0 <= c < self.encoded_size:
                    raise IndexError("column index out of bounds")
                out.append(LcColumn(r.get_encoded_column_without_path(c), self.merkle_tree.get_path(c)))
        return out

    def polynomial_evaluation_response(self, point, columns):
        """The server's answer to an evaluation request from the stored files, without recommitting:
        (result_vector, columns_with_paths), bit-identical to the commitment path's u^T Enc(M) and
        opened columns for left = [1, x^pre, ...].  The raw file gives u^T M (lcpc_pos_left_multiply_bytes)
        and one row encode gives Enc(u^T M) = u^T Enc(M); the columns come from the `.porenc` (canonical
        there, Montgomery limbs here as a commitment opens them) with the `.portree`'s paths."""
        from .lcpc2d import FT63, LcColumn, LigeroEncoding
        from .pos import FT63_MODULUS, form_side_vectors_for_polynomial_evaluation_from_point
        pre, enc = self.pre_encoded_size, self.encoded_size
        left, _ = form_side_vectors_for_polynomial_evaluation_from_point(point, self.rows_written, pre)
        row = np.zeros((enc, 1), np.uint64)
        row[:pre] = np.asarray(self.left_multiply_unencoded_matrix_by_vector(left), dtype=np.uint64).reshape(-1, 1)
        result = LigeroEncoding.new_from_dims(FT63, pre, enc).encode(row)
        cols = [LcColumn(np.array([(int(v) << 64) % FT63_MODULUS for v in np.asarray(c.col).reshape(-1)],
                                  np.uint64).reshape(-1, 1), c.path)
                for c in self.read_full_columns(columns)]
        return result, cols

    # -- batched audits (pos.client_verify_batch_evaluation)
    def batch_evaluation_vectors(self, points) -> np.ndarray:
        """The first message of an audit at m points: the m unencoded vectors v_j = left_j^T M,
        left_j = [1, x_j^pre, ...], as (m, pre) Montgomery words.  The raw file is read once and
        contracted in one pass (lcpc_pos_left_multiply_bytes_many).  It is sent BEFORE the client
        names any column: the order is what makes the batch sound (pos.client_verify_batch_evaluation).
        With one point the vector is left_multiply_unencoded_matrix_by_vector's, and its encode is
        polynomial_evaluation_response's result."""
        from .pos import (form_side_vectors_for_polynomial_evaluation_from_point,
                          left_multiply_unencoded_matrix_by_vectors)
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.uint64)).reshape(-1)
        lefts = np.stack([form_side_vectors_for_polynomial_evaluation_from_point(
            pts[j:j + 1], self.rows_written, self.pre_encoded_size)[0].reshape(-1) for j in range(pts.size)])
        with open(self.unencoded_file_handle, "rb") as f:
            data = f.read(self.total_data_bytes)
        return left_multiply_unencoded_matrix_by_vectors(data, self.pre_encoded_size, lefts)

    def batch_evaluation_columns(self, columns):
        """The second message: read_full_columns(columns) with the values as a commitment opens them
        (Montgomery limbs; the `.porenc` holds canonical ones), one set for all m points."""
        from .lcpc2d import LcColumn
        from .pos import FT63_MODULUS
        return [LcColumn(np.array([(int(v) << 64) % FT63_MODULUS for v in np.asarray(c.col).reshape(-1)],
                                  np.uint64).reshape(-1, 1), c.path)
                for c in self.read_full_columns(columns)]

    # -- checkable reads (pos.client_verify_read)
    def _read_plan(self, byte_start: int, byte_end: int):
        from .pos import read_plan
        return read_plan(self.total_data_bytes, byte_start, byte_end, self.pre_encoded_size)

    def read_rows_response(self, byte_start: int, byte_end: int) -> bytes:
        """The first message of a checkable read: the raw bytes of the whole rows that cover
        [byte_start, byte_end), [row_lo * 7 pre, min(row_hi * 7 pre, file length)).  It is sent BEFORE
        the client names any column: the order is what makes the read sound (pos.client_verify_read)."""
        plan = self._read_plan(byte_start, byte_end)
        rb = self._row_bytes()
        return self.get_unencoded_bytes(plan.row_lo * rb, min(plan.row_hi * rb, self.total_data_bytes))

    def _read_column_rows(self, f, column: int, row_lo: int, row_hi: int) -> np.ndarray:
        """Rows [row_lo, row_hi) of one column: one positioned read of the column-major .porenc."""
        want = (row_hi - row_lo) * WRITTEN_BYTES_WIDTH
        b = os.pread(f.fileno(), want, (column * self.row_capacity + row_lo) * WRITTEN_BYTES_WIDTH)
        if len(b) != want:
            raise EOFError("encoded file shorter than its metadata says")
        return np.frombuffer(b, "<u8").astype(np.uint64)

    def read_opening_response(self, byte_start: int, byte_end: int, columns):
        """The second message: a pos.ReadOpening of the requested columns (strictly increasing, below
        encoded_size) on the leaf chunks that hold the rows of the range -- per column its elements
        there (a contiguous read of the .porenc), the chaining values that cover the rest of the
        column, and its Merkle path.  The cover values come from the chunk cache when the handler
        has one (chunk_cache=True), else from the opened columns read whole; the bytes are the same."""
        from .pos import ReadOpening, segment_covers_from_cache, segment_covers_from_columns
        cols = [int(c) for c in columns]
        if any(b <= a for a, b in zip(cols, cols[1:])) or any(not 0 <= c < self.encoded_size for c in cols):
            raise IndexError("columns must be strictly increasing and below encoded_size")
        plan = self._read_plan(byte_start, byte_end)
        seg_rows = plan.seg_row_hi - plan.seg_row_lo
        segments = np.zeros((len(cols), seg_rows), np.uint64)
        with open(self.encoded_file_handle, "rb") as f:
            for k, c in enumerate(cols):
                segments[k] = self._read_column_rows(f, c, plan.seg_row_lo, plan.seg_row_hi)
            if not cols or plan.n_cover == 0:
                covers = np.zeros((len(cols), plan.n_cover, DIGEST_BYTES), np.uint8)
            elif self.chunk_cache is not None:
                covers = segment_covers_from_cache(self.chunk_cache, cols, plan.chunk_lo, plan.chunk_hi)
            else:
                whole = np.stack([self._read_column_rows(f, c, 0, self.rows_written) for c in cols])
                covers = segment_covers_from_columns(whole, self.rows_written, plan.chunk_lo, plan.chunk_hi)
        return ReadOpening(segments, covers, [self.merkle_tree.get_path(c) for c in cols])

    # -- re-encoding
    def _reencode_rows(self, row_lo: int, row_hi: int) -> None:
        """Rows [row_lo, row_hi) from the raw file into the .porenc (one batched GPU pass)."""
        if row_hi <= row_lo:
            return
        rb = self._row_bytes()
        data = self.get_unencoded_bytes(row_lo * rb, min(row_hi * rb, self.total_data_bytes))
        img_bytes = self.row_capacity * self.encoded_size * WRITTEN_BYTES_WIDTH
        with open(self.encoded_file_handle, "r+b") as f:
            if os.fstat(f.fileno()).st_size < img_bytes:
                raise ValueError("encoded file shorter than row_capacity * encoded_size elements")
            mm = mmap.mmap(f.fileno(), img_bytes)
            try:
                arr = np.frombuffer(mm, np.uint8)
                p, keep = _bytes_ptr(data)
                _raise(N.load().lcpc_pos_reencode_rows(p, len(data), self.pre_encoded_size, self.encoded_size,
                                                       row_lo, _u8(arr), self.row_capacity))
                del arr
                mm.flush()
            finally:
                mm.close()

    def reencode_row(self, row_index: int) -> None:
        """:380-402"""
        if not row_index < self.rows_written:
            raise IndexError("cannot reencode a row that is out of bounds")
        self._reencode_rows(row_index, row_index + 1)

    def reencode_unencoded_file(self) -> None:
        """:406-462 -- the whole raw file through the GPU writer again."""
        self.total_data_bytes = os.path.getsize(self.unencoded_file_handle)
        with open(self.unencoded_file_handle, "rb") as raw, open(self.encoded_file_handle, "w+b") as tf:
            w = EncodedFileWriter(self.pre_encoded_size, self.encoded_size, self.total_data_bytes, tf)
            if self.total_data_bytes:
                w.push_bytes(raw.read())
            m, tree = w.finalize_to_merkle_tree(keep_chunk_cvs=self.chunk_cache is not None)
        self.write_tree(tree)
        self.pre_encoded_size, self.encoded_size = m.pre_encoded_size, m.encoded_size
        self.total_data_bytes, self.row_capacity, self.rows_written = m.bytes_of_data, m.row_capacity, m.rows_written
        self._write_metadata()
        self.merkle_tree = tree
        if self.chunk_cache is not None:  # the writer's own CVs: no second pass
            write_chunk_cv_sidecar(self.chunk_cv_file_handle, self.encoded_size, self.rows_written, tree.root(),
                                   w.chunk_cvs)
            self.chunk_cache.close()
            self.chunk_cache = ColumnChunkCache.from_cvs(w.chunk_cvs, self.encoded_size, self.rows_written)

    def edit_bytes(self, byte_start: int, unencoded_bytes_to_add: bytes) -> Tuple[bytes, MerkleTree]:
        """:279-333 -- returns the bytes that were replaced and the new tree."""
        if not os.path.isfile(self.unencoded_file_handle):
            raise FileNotFoundError("no unencoded file found!")
        n = len(unencoded_bytes_to_add)
        if byte_start + n > self.total_data_bytes:
            raise ValueError("can't edit more bytes than there are in the file!")
        with open(self.unencoded_file_handle, "r+b") as f:
            f.seek(byte_start)
            original = f.read(n)
            f.seek(byte_start)
            f.write(unencoded_bytes_to_add)
        rb = self._row_bytes()
        row_lo, row_hi = byte_start // rb, -(-(byte_start + n) // rb)
        self._reencode_rows(row_lo, row_hi)
        if self.chunk_cache is not None:
            return original, self._update_chunk_cache(row_lo, max(row_lo, row_hi))
        return original, self.recalculate_merkle_tree()

    def append_bytes(self, bytes_to_add: bytes) -> MerkleTree:
        """:335-366"""
        with open(self.unencoded_file_handle, "ab") as f:
            f.write(bytes_to_add)
        rb = self._row_bytes()
        start_row = self.total_data_bytes // rb
        end_row = -(-(self.total_data_bytes + len(bytes_to_add)) // rb)
        if end_row > self.row_capacity:
            with open(self.encoded_file_handle, "r+b") as f:
                self._reader(f).set_new_capacity(end_row * 2)
            self.row_capacity = end_row * 2
        self.total_data_bytes += len(bytes_to_add)
        self.rows_written = end_row
        self._reencode_rows(start_row, end_row)
        # (the capacity growth above re-lays the image but changes no value: the cache stays valid)
        if self.chunk_cache is not None:
            tree = self._update_chunk_cache(start_row, max(start_row, end_row))
        else:
            tree = self.recalculate_merkle_tree()
        self._write_metadata()
        return tree

    def reshape(self, new_pre_encoded_columns: int, new_encoded_columns: int
                ) -> Tuple[EncodedFileMetadata, MerkleTree]:
        """:224-276 (convert_unencoded_file with the new shape)."""
        with open(self.unencoded_file_handle, "r+b") as f:
            m, tree = EncodedFileWriter.convert_unencoded_file(
                f, self.encoded_file_handle, self.merkle_tree_file_handle, self.metadata_file_handle,
                new_pre_encoded_columns, new_encoded_columns,
                self.chunk_cv_file_handle if self.chunk_cache is not None else None)
        self.pre_encoded_size, self.encoded_size = new_pre_encoded_columns, new_encoded_columns
        self.rows_written, self.row_capacity = m.rows_written, m.row_capacity
        self.merkle_tree = tree
        self._write_metadata()  # keeps the ulid, which convert_unencoded_file's metadata lacks
        if self.chunk_cache is not None:
            self._attach_chunk_cache()  # the sidecar that pass just wrote, for the new shape
        m.ulid = self.file_ulid
        return m, tree

    # -- tree and metadata
    def recalculate_merkle_tree(self) -> MerkleTree:
        """:474-481 (process_file_to_merkle_tree on the GPU)."""
        with open(self.encoded_file_handle, "rb") as f:
            tree = self._reader(f).process_file_to_merkle_tree()
        self.merkle_tree = tree
        self.write_tree(tree)
        return tree

    def write_tree(self, tree: MerkleTree) -> None:
        if len(tree) != self.encoded_size * 2 - 1:
            raise ValueError("this Merkle tree is the incorrect size")
        with open(self.merkle_tree_file_handle, "wb") as f:
            write_tree_to_file(f, tree)

    def _write_metadata(self) -> None:
        with open(self.metadata_file_handle, "wb") as f:
            self.get_encoded_metadata().write_to_file(f)

    def verify_all_files_agree(self) -> None:
        """:505-541: the tree from the .porenc, and the tree of a fresh encode of the raw file,
        must both equal the stored tree (and the raw file must hold total_data_bytes)."""
        if self.recalculate_tree_only() != self.merkle_tree:
            raise AssertionError("the encoded file's tree differs from the stored tree")
        n = os.path.getsize(self.unencoded_file_handle)
        if n != self.total_data_bytes:
            raise AssertionError("raw file length differs from the metadata")
        rows = -(-(-(-n // DATA_BYTE_CAPACITY)) // self.pre_encoded_size)
        img = np.zeros(max(rows, 1) * self.encoded_size * WRITTEN_BYTES_WIDTH, np.uint8)
        data = np.fromfile(self.unencoded_file_handle, np.uint8)
        tree = np.zeros((2 * self.encoded_size - 1, DIGEST_BYTES), np.uint8)
        out_rows = C.c_size_t()
        _raise(N.load().lcpc_pos_encode_file(_u8(data), n, self.pre_encoded_size, self.encoded_size, max(rows, 1),
                                             _u8(img), _u8(tree), C.byref(out_rows)))
        if MerkleTree(tree) != self.merkle_tree:
            raise AssertionError("the raw file's re-encoded tree differs from the stored tree")
        if self.chunk_cache is not None:
            if self.chunk_cache.tree() != self.merkle_tree:
                raise AssertionError("the chunk-CV cache folds to a tree that differs from the stored tree")
            fresh = self._rebuild_chunk_cache()
            try:
                if not np.array_equal(fresh.copy_cvs(), self.chunk_cache.copy_cvs()):
                    raise AssertionError("the chunk-CV cache differs from one rebuilt from the encoded file")
            finally:
                fresh.close()

    def recalculate_tree_only(self) -> MerkleTree:
        with open(self.encoded_file_handle, "rb") as f:
            return self._reader(f).process_file_to_merkle_tree()

    # -- scrub and repair (no counterpart in the reference, whose verify_all_files_agree can only
    # say that the trees differ): the damaged `.porenc` columns are located against the stored
    # leaves and recomputed from the code's own redundancy
    def _stored_tree(self) -> MerkleTree:
        """The `.portree` as it is on disk now (damage may be newer than this handler)."""
        with open(self.merkle_tree_file_handle, "rb") as f:
            data = f.read()
        want = (2 * self.encoded_size - 1) * DIGEST_BYTES
        if len(data) != want:
            raise UnrecoverableError("the stored tree file has the wrong length")
        return MerkleTree(np.frombuffer(data, np.uint8).copy())

    def _raw_file_tree(self) -> Optional[MerkleTree]:
        """The tree of a fresh encode of the raw file (a digest-only writer: no image is kept);
        None if the raw file is missing or does not hold total_data_bytes."""
        try:
            if os.path.getsize(self.unencoded_file_handle) != self.total_data_bytes:
                return None
            data = np.fromfile(self.unencoded_file_handle, np.uint8)
        except OSError:
            return None
        lib, h = N.load(), N.vp()
        _raise(lib.lcpc_pos_writer_new(self.pre_encoded_size, self.encoded_size, None, 0, 0, C.byref(h)))
        try:
            _raise(lib.lcpc_pos_writer_push_bytes(h, _u8(data), data.size))
            tree = np.zeros((2 * self.encoded_size - 1, DIGEST_BYTES), np.uint8)
            rows, nbytes = C.c_size_t(), C.c_size_t()
            _raise(lib.lcpc_pos_writer_finalize(h, None, _u8(tree), C.byref(rows), C.byref(nbytes)))
        finally:
            lib.lcpc_pos_writer_free(h)
        return MerkleTree(tree)

    def _scrub_state(self, expected_root: Optional[bytes]):
        tree = self._stored_tree()
        w = self.encoded_size
        consistent = MerkleTree.new(tree.digests[:w]) == tree
        with open(self.encoded_file_handle, "rb") as f:
            status, digests = self._reader(f)._scrub(tree.digests[:w])
        raw_tree = self._raw_file_tree()
        report = ScrubReport(
            bad_columns=[int(c) for c in np.flatnonzero(status)],
            noncanonical_columns=[int(c) for c in np.flatnonzero(status == 2)],
            tree_consistent=bool(consistent),
            root_ok=None if expected_root is None else tree.root() == bytes(expected_root),
            raw_ok=raw_tree is not None and raw_tree == tree)
        return report, tree, digests, raw_tree

    def _locate_into(self, report: ScrubReport) -> np.ndarray:
        """Fills report.located_columns / unlocatable_rows from the code's own syndromes."""
        with open(self.encoded_file_handle, "rb") as f:
            status, n_unloc = self._reader(f).locate_damaged_columns()
        report.located_columns = [int(c) for c in np.flatnonzero(status)]
        report.unlocatable_rows = n_unloc
        return status

    def _scrub_state_located(self, expected_root: Optional[bytes]) -> ScrubReport:
        """scrub(locate=True): as _scrub_state, but a tree file that is missing or has the wrong
        length is a finding (no bad_columns, tree_consistent False), not an error."""
        try:
            report = self._scrub_state(expected_root)[0]
        except (UnrecoverableError, OSError):
            report = ScrubReport(bad_columns=[], noncanonical_columns=[], tree_consistent=False,
                                 root_ok=None if expected_root is None else False, raw_ok=False)
        return self._locate_report(report)

    def _locate_report(self, report: ScrubReport) -> ScrubReport:
        """The locate half of scrub(locate=True) over a report of the tree's findings."""
        try:
            with open(self.encoded_file_handle, "rb") as f:
                located = self._reader(f).locate_damaged_columns()
        except UnrecoverableError:  # more non-canonical columns than the code's redundancy
            located = None
        return self._fill_locate_report(report, located)

    def _fill_locate_report(self, report: ScrubReport, located) -> ScrubReport:
        """located: (col_status, unlocatable_rows) of locate_damaged_columns with no known columns (this
        file's own call, or the grouped locate of repair_files), or None where that is
        unrecoverable."""
        if located is None:
            report.located_columns, report.unlocatable_rows = [], self.rows_written
            return report
        status, n_unloc = located
        report.located_columns = [int(c) for c in np.flatnonzero(status)]
        report.unlocatable_rows = int(n_unloc)
        if not report.bad_columns and not report.tree_consistent:
            report.noncanonical_columns = [int(c) for c in np.flatnonzero(status == 2)]
        return report

    def scrub(self, expected_root: Optional[bytes] = None, locate: bool = False) -> ScrubReport:
        """Read-only health check of the four files against each other (and against expected_root,
        the root the client holds, if given): which `.porenc` columns differ from their stored
        leaves, whether the stored tree refolds, whether the raw file still encodes to it.
        locate=True also asks the code itself (EncodedFileReader.locate_damaged_columns): the report
        gains located_columns and unlocatable_rows, and a tree file that is missing or has the wrong
        length no longer raises (bad_columns is then empty and tree_consistent False)."""
        if locate:
            return self._scrub_state_located(expected_root)
        return self._scrub_state(expected_root)[0]

    def _repair_located(self, expected_root: Optional[bytes]) -> ScrubReport:
        """repair(locate=True) where the tree cannot say where the damage is: the columns the code's
        syndromes name are recomputed, and the result is written only if the tree over all column
        digests folds to expected_root -- or, with no expected_root, equals the tree of a fresh
        encode of the raw file.  The code's self-consistency alone is never an anchor."""
        report = self._scrub_state_located(expected_root)
        raw_tree = self._raw_file_tree()

        def recompute(bad):
            w = self.encoded_size
            with open(self.encoded_file_handle, "rb") as f:
                reader = self._reader(f)
                cols, rdig = reader.repair_columns(bad) if bad else (None, None)
                # the digests of every column as the file holds it; the located ones are replaced below
                _, digests = reader._scrub(np.zeros((w, DIGEST_BYTES), np.uint8))
            digests = digests.copy()
            if bad:
                digests[bad] = rdig
            return cols, MerkleTree.new(digests)
        return self._apply_located(expected_root, report, raw_tree, recompute)

    def _apply_located(self, expected_root: Optional[bytes], report: ScrubReport, raw_tree: Optional[MerkleTree],
                       recompute) -> ScrubReport:
        """The trust rule and all writes of _repair_located over a located scrub state (this file's own, or
        the grouped passes' of repair_files).  recompute(located columns) gives (their recomputed columns or
        None with none located, the tree over the digests of all columns with the recomputed ones in place):
        this file's own calls, or what a grouped repair already returned."""
        w, pre = self.encoded_size, self.pre_encoded_size
        if report.unlocatable_rows:
            raise UnrecoverableError(f"{report.unlocatable_rows} rows hold more wrong elements than can be located")
        bad = report.located_columns
        if len(bad) > w - pre:
            raise UnrecoverableError(f"{len(bad)} columns located as damaged (at most {w - pre} can be recomputed)")
        if expected_root is None and raw_tree is None:
            raise UnrecoverableError("no expected_root was given and the raw file cannot vouch for the repair")
        cols, new_tree = recompute(bad)
        if expected_root is not None:
            if new_tree.root() != bytes(expected_root):
                raise UnrecoverableError("the located repair does not fold to expected_root")
        elif raw_tree != new_tree:
            raise UnrecoverableError("the located repair and the raw file do not agree")
        done = ["located"]
        if bad:
            wb, wrote = WRITTEN_BYTES_WIDTH, False
            with open(self.encoded_file_handle, "r+b") as f:
                for k, c in enumerate(bad):
                    new = cols[k].tobytes()
                    f.seek(c * self.row_capacity * wb)
                    if f.read(len(new)) != new:
                        f.seek(c * self.row_capacity * wb)
                        f.write(new)
                        wrote = True
                f.flush()
            if wrote:
                done.append("columns")
        try:
            with open(self.merkle_tree_file_handle, "rb") as f:
                tree_same = f.read() == new_tree.to_bytes()
        except OSError:
            tree_same = False
        if not tree_same:
            self.write_tree(new_tree)
            done.append("tree")
        self.merkle_tree = new_tree
        if raw_tree is None or raw_tree != new_tree:
            with open(self.encoded_file_handle, "rb") as f:
                data = self._reader(f)._decode(0, self.rows_written) if self.rows_written else b""
            with open(self.unencoded_file_handle, "wb") as f:
                f.write(data[:self.total_data_bytes])
            done.append("raw")
        if self.chunk_cache is not None:
            cache = self._rebuild_chunk_cache()
            write_chunk_cv_sidecar(self.chunk_cv_file_handle, w, self.rows_written, cache.tree().root(),
                                   cache.copy_cvs())
            self.chunk_cache.close()
            self.chunk_cache = cache
        report.repaired_from = "+".join(done)
        return report

    def repair(self, expected_root: Optional[bytes] = None, locate: bool = False) -> ScrubReport:
        """Mend what scrub finds; see _repair_by_tree.  locate=True: that path runs first, unchanged;
        only where it raises UnrecoverableError -- the tree file is missing or has the wrong length,
        it does not refold and no expected_root was given, or the leaves name too many columns and the
        raw file does not verify -- the damaged columns are located by the code's own syndromes
        (_repair_located; repaired_from then starts with "located").  That result is written only
        if it verifies against expected_root, or, without one, against a fresh encode of the raw
        file; otherwise UnrecoverableError with every file byte for byte what it was."""
        if not locate:
            return self._repair_by_tree(expected_root)
        try:
            return self._repair_by_tree(expected_root)
        except (UnrecoverableError, FileNotFoundError):
            return self._repair_located(expected_root)

    def _repair_by_tree(self, expected_root: Optional[bytes] = None) -> ScrubReport:
        """Mend what scrub finds.  Everything written is first verified against the trust anchor:
        expected_root if given, otherwise the stored tree's root provided the stored tree is
        self-consistent.  Up to encoded_size - pre_encoded_size damaged columns are recomputed from
        the others (erasure decoding); they -- and a tree rebuilt from the column digests, where the
        stored one was what was damaged -- are written only if the resulting root is the anchor.
        With more damage the raw file is encoded again, accepted only if its root is the anchor.  A
        sound `.porenc` rewrites a damaged raw file from its decode.  UnrecoverableError if nothing
        verifies; every file is then byte for byte what it was."""
        return self._apply_repair(expected_root, *self._scrub_state(expected_root))

    def _apply_repair(self, expected_root: Optional[bytes], report: ScrubReport, tree: MerkleTree,
                      digests: np.ndarray, raw_tree: Optional[MerkleTree], repaired=None) -> ScrubReport:
        """The trust rules of _repair_by_tree over a scrub state (_scrub_state's, or the grouped scrub's
        of repair_files).  repaired: (columns, digests, tree digests) of report.bad_columns from a grouped
        repair over `digests` as leaves; None: they are recomputed here, by this file's own call."""
        w, pre = self.encoded_size, self.pre_encoded_size
        if expected_root is not None:
            anchor = bytes(expected_root)
        elif report.tree_consistent:
            anchor = tree.root()
        else:
            raise UnrecoverableError("the stored tree is not self-consistent and no expected_root was given")
        done: List[str] = []
        bad = report.bad_columns
        new_tree, cols = None, None
        if len(bad) <= w - pre:
            try:
                rebuilt = None
                if bad:
                    if repaired is not None:
                        cols, rdig, rebuilt = repaired
                    else:
                        with open(self.encoded_file_handle, "rb") as f:
                            cols, rdig = self._reader(f).repair_columns(bad)
                    digests = digests.copy()
                    digests[bad] = rdig
                # a repaired column whose digest is not its leaf is a damaged leaf (or damage this
                # cannot mend): either way only a tree over the digests that folds to the anchor counts
                cand = tree if (report.tree_consistent and np.array_equal(digests, tree.digests[:w])) \
                    else MerkleTree(rebuilt) if rebuilt is not None else MerkleTree.new(digests)
                if cand.root() == anchor:
                    new_tree = cand
            except UnrecoverableError:
                new_tree = None
        if new_tree is not None:
            if bad:  # (a column whose leaf was what was damaged repairs to itself: nothing to write)
                wb, wrote = WRITTEN_BYTES_WIDTH, False
                with open(self.encoded_file_handle, "r+b") as f:
                    for k, c in enumerate(bad):
                        new = cols[k].tobytes()
                        f.seek(c * self.row_capacity * wb)
                        if f.read(len(new)) != new:
                            f.seek(c * self.row_capacity * wb)
                            f.write(new)
                            wrote = True
                    f.flush()
                if wrote:
                    done.append("columns")
            if new_tree != tree:
                self.write_tree(new_tree)
                done.append("tree")
            self.merkle_tree = new_tree
            if raw_tree is None or raw_tree != new_tree:  # the encoded file is sound, the raw one is not
                with open(self.encoded_file_handle, "rb") as f:
                    data = self._reader(f)._decode(0, self.rows_written) if self.rows_written else b""
                with open(self.unencoded_file_handle, "wb") as f:
                    f.write(data[:self.total_data_bytes])
                done.append("raw")
        elif raw_tree is not None and raw_tree.root() == anchor:
            self.reencode_unencoded_file()  # (rebuilds the chunk-CV cache itself)
            done = ["reencode"]
        else:
            raise UnrecoverableError(
                f"{len(bad)} damaged columns (at most {w - pre} can be recomputed) and the raw file "
                "does not encode to the trusted root")
        if self.chunk_cache is not None and done and done != ["reencode"]:
            cache = self._rebuild_chunk_cache()
            write_chunk_cv_sidecar(self.chunk_cv_file_handle, w, self.rows_written, cache.tree().root(),
                                   cache.copy_cvs())
            self.chunk_cache.close()
            self.chunk_cache = cache
        report.repaired_from = "+".join(done) if done else None
        return report

    def delete_all_files(self) -> None:
        """:678-694"""
        for p in (self.unencoded_file_handle, self.encoded_file_handle, self.merkle_tree_file_handle,
                  self.metadata_file_handle):
            os.remove(p)
        if self.chunk_cache is not None:
            self.chunk_cache.close()
            self.chunk_cache = None
        if os.path.isfile(self.chunk_cv_file_handle):  # (also one an earlier cached handler left)
            os.remove(self.chunk_cv_file_handle)
        d = os.path.dirname(self.unencoded_file_handle)
        if not os.listdir(d):
            os.rmdir(d)


# -- grouped scrub
# files mapped at once by scrub_files: an image and a raw file each hold a descriptor while their batch runs
_SCRUB_FILES_BATCH = 192


def _close_map(mm) -> None:
    try:
        mm.close()
    except BufferError:  # an in-flight exception's traceback still holds a view
        pass


_OWN_LOCATE = object()   # _locate_grouped: the grouped pass gave no answer; the file's handler locates


def _locate_grouped(handlers, images, noncanon, keys) -> dict:
    """One lcpc_pos_locate_files_grouped call over mapped images with the columns the scrub found to hold a
    word that is not < p as known columns.  {key: what FileHandler._fill_locate_report takes} -- (col_status
    with those columns as 2, as the file's own locate_damaged_columns() names them, unlocatable rows), or
    None where the call is unrecoverable for the file."""
    from .pos import locate_files_grouped
    if not handlers:
        return {}
    res = locate_files_grouped(images, [h.pre_encoded_size for h in handlers], [h.encoded_size for h in handlers],
                               [h.rows_written for h in handlers], [h.row_capacity for h in handlers], noncanon)
    out = {}
    for key, o in zip(keys, res):
        if o["status"] == LCPC_ERR_UNRECOVERABLE:
            out[key] = None
        elif o["status"]:
            out[key] = _OWN_LOCATE
        else:
            status = o["col_status"].copy()
            status[status == 3] = 2
            out[key] = (status, o["n_unlocatable_rows"])
    return out


def _scrub_files_batch(handlers, roots, locate: bool, states: Optional[list] = None) -> List[ScrubReport]:
    """states (repair_files): a list that gets, per file, what FileHandler._scrub_state returns beside the
    report -- (stored tree, column digests, raw file's tree or None) -- and the columns that hold a word that
    is not < p; the stored tree is None for a file without a usable tree file, which is then no error here
    either (its digests are those of the columns as they stand, its raw file is still encoded)."""
    from .pos import encode_files_grouped_into, scrub_files_grouped
    trees: List[Optional[MerkleTree]] = []
    for h in handlers:
        try:
            trees.append(h._stored_tree())
        except (UnrecoverableError, OSError):
            # scrub() raises; scrub(locate=True) reports a file without a usable tree; repair_files asks its handler
            if not locate and states is None:
                raise
            trees.append(None)
    files, maps, images = [], [], []
    try:
        for h in handlers:
            need = h.row_capacity * h.encoded_size * WRITTEN_BYTES_WIDTH
            f = open(h.encoded_file_handle, "rb")
            files.append(f)
            if os.fstat(f.fileno()).st_size < need:
                raise ValueError("encoded file shorter than row_capacity * encoded_size elements")
            mm = mmap.mmap(f.fileno(), need, access=mmap.ACCESS_READ) if need else None
            maps.append(mm)
            images.append(np.frombuffer(mm, np.uint8) if need else None)
        res = scrub_files_grouped(
            images, [h.pre_encoded_size for h in handlers], [h.encoded_size for h in handlers],
            [h.rows_written for h in handlers], [h.row_capacity for h in handlers],
            [None if t is None else t.digests for t in trees],
            [None if t is None else r for t, r in zip(trees, roots)], want_digests=states is not None)
    finally:
        del images
        for mm in maps:
            if mm is not None:
                _close_map(mm)
        for f in files:
            f.close()
    # raw_ok: one grouped ingest of the raw files that can still match, trees only
    raw_trees: List[Optional[np.ndarray]] = [None] * len(handlers)
    files, maps, datas, who = [], [], [], []
    try:
        for i, h in enumerate(handlers):
            if trees[i] is None and states is None:
                continue
            try:
                if os.path.getsize(h.unencoded_file_handle) != h.total_data_bytes:
                    continue
                f = open(h.unencoded_file_handle, "rb")
            except OSError:
                continue
            files.append(f)
            mm = mmap.mmap(f.fileno(), h.total_data_bytes, access=mmap.ACCESS_READ) if h.total_data_bytes else None
            maps.append(mm)
            datas.append(np.frombuffer(mm, np.uint8) if mm is not None else np.zeros(0, np.uint8))
            who.append(i)
        if who:
            enc = encode_files_grouped_into(datas, [handlers[i].pre_encoded_size for i in who],
                                            [handlers[i].encoded_size for i in who], None, None, True, False, False)
            for i, o in zip(who, enc):
                raw_trees[i] = o["tree"]
    finally:
        del datas
        for mm in maps:
            if mm is not None:
                _close_map(mm)
        for f in files:
            f.close()
    out = []
    for h, tree, root, r, raw in zip(handlers, trees, roots, res, raw_trees):
        status = r["status"]
        if tree is None:
            report = ScrubReport(bad_columns=[], noncanonical_columns=[], tree_consistent=False,
                                 root_ok=None if root is None else False, raw_ok=False)
        else:
            report = ScrubReport(
                bad_columns=[int(c) for c in np.flatnonzero(status)],
                noncanonical_columns=[int(c) for c in np.flatnonzero(status == 2)],
                tree_consistent=bool(r["tree_consistent"]),
                root_ok=None if root is None else bool(r["root_ok"]),
                raw_ok=raw is not None and np.array_equal(raw, tree.digests))
        if locate:
            if r["n_dirty_rows"] == 0 and not (status == 2).any():
                # every row a codeword and every word canonical: what the locator returns for such a file
                report.located_columns, report.unlocatable_rows = [], 0
            else:
                h._locate_report(report)
        out.append(report)
        if states is not None:
            states.append((tree, r["digests"], None if raw is None else MerkleTree(raw),
                           [int(c) for c in np.flatnonzero(status == 2)]))
    return out


def scrub_files(handlers, expected_roots=None, locate: bool = False) -> List[ScrubReport]:
    """FileHandler.scrub for many stored files in grouped passes: entry i equals
    handlers[i].scrub(expected_root=expected_roots[i], locate=locate) field by field.  Every `.porenc` is
    mapped and every `.portree` read; column statuses, the trees' consistency, their roots and the rows
    that are no codewords come from lcpc_pos_scrub_files_grouped, and raw_ok from one grouped ingest of the
    raw files (trees only) per batch of files.  A tree file that is missing or of the wrong length raises
    as scrub does with locate=False and is the finding scrub(locate=True) reports otherwise.  With
    locate=True a file whose rows are all codewords and whose words are all canonical needs no per-file
    device call; every other file goes through its handler's own locate.  A clean store is scrubbed, locate
    included, with launches per staging group of files, not per file."""
    handlers = list(handlers)
    roots = [None] * len(handlers) if expected_roots is None else list(expected_roots)
    if len(roots) != len(handlers):
        raise ValueError("expected_roots must have one entry per handler")
    out: List[ScrubReport] = []
    for lo in range(0, len(handlers), _SCRUB_FILES_BATCH):
        out += _scrub_files_batch(handlers[lo:lo + _SCRUB_FILES_BATCH], roots[lo:lo + _SCRUB_FILES_BATCH], locate)
    return out


# -- grouped repair
def _map_images(handlers):
    """(files, maps, images) of the handlers' `.porenc` files mapped read-only; _unmap gives them back"""
    files, maps, images = [], [], []
    try:
        for h in handlers:
            need = h.row_capacity * h.encoded_size * WRITTEN_BYTES_WIDTH
            f = open(h.encoded_file_handle, "rb")
            files.append(f)
            mm = mmap.mmap(f.fileno(), need, access=mmap.ACCESS_READ) if need else None
            maps.append(mm)
            images.append(np.frombuffer(mm, np.uint8) if need else None)
    except BaseException:
        _unmap(files, maps, images)
        raise
    return files, maps, images


def _unmap(files, maps, images) -> None:
    del images[:]
    for mm in maps:
        if mm is not None:
            _close_map(mm)
    for f in files:
        f.close()


def _repair_files_batch(handlers, roots, locate: bool) -> list:
    from .pos import repair_files_grouped
    states: list = []
    reports = _scrub_files_batch(handlers, roots, False, states)
    # one grouped repair for the files the tree can mend: an anchor, and 1 .. enc - pre bad columns
    who = []
    for i, (h, root, report, st) in enumerate(zip(handlers, roots, reports, states)):
        if st[0] is not None and (root is not None or report.tree_consistent) and \
                1 <= len(report.bad_columns) <= h.encoded_size - h.pre_encoded_size:
            who.append(i)
    repaired = {}
    files, maps, images = _map_images([handlers[i] for i in who])
    try:
        if who:
            res = repair_files_grouped(
                images, [handlers[i].pre_encoded_size for i in who], [handlers[i].encoded_size for i in who],
                [handlers[i].rows_written for i in who], [handlers[i].row_capacity for i in who],
                [reports[i].bad_columns for i in who], [states[i][1] for i in who], want_cols=True, want_tree=True)
            for i, o in zip(who, res):
                if o["status"] == 0:     # (a file the grouped pass could not mend takes its own handler's path)
                    repaired[i] = (o["cols"], o["digests"], o["tree"])
    finally:
        _unmap(files, maps, images)
    out: list = [None] * len(handlers)
    fallback = []            # locate=True: the files whose tree path raised what repair() answers by locating
    for i, (h, root, report, st) in enumerate(zip(handlers, roots, reports, states)):
        try:
            if st[0] is None:       # no usable tree file: the handler's own path says what that means
                if locate:
                    try:
                        h._stored_tree()
                    except (UnrecoverableError, FileNotFoundError):
                        fallback.append(i)
                        continue
                out[i] = h.repair(expected_root=root, locate=locate)
                continue
            try:
                out[i] = h._apply_repair(root, report, *st[:3], repaired=repaired.get(i))
            except UnrecoverableError:
                if not locate:
                    raise
                fallback.append(i)
        except (UnrecoverableError, OSError) as e:
            out[i] = e
    if fallback:
        _repair_located_grouped(handlers, roots, reports, states, fallback, out)
    return out


def _located_is_repairable(h, report, root, raw_tree) -> bool:
    """whether FileHandler._apply_located gets as far as recomputing the located columns (none among them:
    the tree over the columns as they stand)"""
    return not report.unlocatable_rows and \
        len(report.located_columns) <= h.encoded_size - h.pre_encoded_size and (root is not None or raw_tree is not None)


def _repair_located_grouped(handlers, roots, reports, states, who, out) -> None:
    """FileHandler._repair_located for the files `who` of a batch in grouped passes: one grouped locate (the
    columns the scrub found to hold a word that is not < p as known columns), one grouped repair with the
    located columns as the erasure set, the scrub's digests of all columns as leaves and the tree wanted,
    then FileHandler._apply_located per file -- the trust rule and all writes -- against expected_root or
    the raw file's tree of the batch's grouped ingest.  A file the grouped passes cannot answer takes its
    handler's own _repair_located."""
    from .pos import repair_files_grouped
    try:
        files, maps, images = _map_images([handlers[i] for i in who])
    except OSError:
        for i in who:        # a `.porenc` that cannot be opened: every file says for itself what it raises
            try:
                out[i] = handlers[i]._repair_located(roots[i])
            except (UnrecoverableError, OSError) as e:
                out[i] = e
        return
    mended = {}
    try:
        located = _locate_grouped([handlers[i] for i in who], images, [states[i][3] for i in who], who)
        rep, rep_images = [], []
        for i, img in zip(who, images):
            h = handlers[i]
            if located[i] is _OWN_LOCATE:
                continue
            h._fill_locate_report(reports[i], located[i])
            if _located_is_repairable(h, reports[i], roots[i], states[i][2]):
                rep.append(i)
                rep_images.append(img)
        if rep:
            res = repair_files_grouped(
                rep_images, [handlers[i].pre_encoded_size for i in rep], [handlers[i].encoded_size for i in rep],
                [handlers[i].rows_written for i in rep], [handlers[i].row_capacity for i in rep],
                [reports[i].located_columns for i in rep], [states[i][1] for i in rep], want_cols=True, want_tree=True)
            for i, o in zip(rep, res):
                if o["status"] == 0:
                    mended[i] = (o["cols"], MerkleTree(o["tree"]))
        del rep_images
    finally:
        _unmap(files, maps, images)
    for i in who:
        h, report = handlers[i], reports[i]
        try:
            if located[i] is _OWN_LOCATE or \
                    (i not in mended and _located_is_repairable(h, report, roots[i], states[i][2])):
                out[i] = h._repair_located(roots[i])        # the grouped passes gave no answer
                continue

            def recompute(bad, i=i):
                cols, tree = mended[i]
                return (cols if bad else None), tree
            out[i] = h._apply_located(roots[i], report, states[i][2], recompute)
        except (UnrecoverableError, OSError) as e:
            out[i] = e


def repair_files(handlers, expected_roots=None, locate: bool = False) -> list:
    """FileHandler.repair for many stored files in grouped passes: entry i is the ScrubReport that
    handlers[i].repair(expected_root=expected_roots[i], locate=locate) returns, field by field, or the
    exception (UnrecoverableError, or the OSError of a missing file) that call would raise; the other
    files are still repaired, and afterwards every file on disk is byte for byte what the per-file loop
    leaves.  The scrub state of a batch comes from the grouped scrub (scrub_files' passes); every file
    with an anchor and between 1 and enc - pre bad columns goes through one
    lcpc_pos_repair_files_grouped call per batch, with the scrub's digests as leaves and the tree
    wanted; FileHandler._apply_repair then applies _repair_by_tree's trust rules and writes.  A file
    the grouped repair cannot mend (too many columns, no anchor, an unrecoverable verdict, no usable tree
    file with locate=False) takes its own handler's calls from there.  With locate=True the files whose tree
    path raised -- a tree file that is missing, truncated or overwritten among them -- go through one
    grouped locate and one grouped repair per batch (_repair_located_grouped) and
    FileHandler._apply_located, the trust rule and the writes of _repair_located."""
    handlers = list(handlers)
    roots = [None] * len(handlers) if expected_roots is None else list(expected_roots)
    if len(roots) != len(handlers):
        raise ValueError("expected_roots must have one entry per handler")
    out: list = []
    for lo in range(0, len(handlers), _SCRUB_FILES_BATCH):
        out += _repair_files_batch(handlers[lo:lo + _SCRUB_FILES_BATCH], roots[lo:lo + _SCRUB_FILES_BATCH], locate)
    return out


# -- grouped audits
def answer_evaluation_requests(requests):
    """A server's queue of evaluation requests over different stored files, answered together:
    `requests` is a sequence of (FileHandler, point, columns), the result the list of (result_vector,
    columns_with_paths), entry i bit-identical to requests[i][0].polynomial_evaluation_response(point,
    columns).  The same handler may appear in several requests (its raw file is read once).

    The raw files go through one grouped contraction (lcpc_pos_left_multiply_bytes_grouped: launches
    per staging group, not per file), the vectors through one encode_rows per distinct (pre, enc), and
    the opened columns from canonical to Montgomery words in the library (lcpc_field_to_montgomery),
    not in a Python loop over elements."""
    from .lcpc2d import FT63, LcColumn, LigeroEncoding
    from .pos import (field_to_montgomery, form_side_vectors_for_polynomial_evaluation_from_point,
                      left_multiply_unencoded_matrices_by_vectors)
    reqs = [(fh, point, list(columns)) for fh, point, columns in requests]
    if not reqs:
        return []
    raw = {}
    for fh, _, _ in reqs:
        if id(fh) not in raw:
            with open(fh.unencoded_file_handle, "rb") as f:
                raw[id(fh)] = f.read(fh.total_data_bytes)
    lefts = [form_side_vectors_for_polynomial_evaluation_from_point(point, fh.rows_written, fh.pre_encoded_size)[0]
             for fh, point, _ in reqs]
    vectors = left_multiply_unencoded_matrices_by_vectors([raw[id(fh)] for fh, _, _ in reqs],
                                                          [fh.pre_encoded_size for fh, _, _ in reqs], lefts)
    by_dims = {}
    for i, (fh, _, _) in enumerate(reqs):
        by_dims.setdefault((fh.pre_encoded_size, fh.encoded_size), []).append(i)
    results = [None] * len(reqs)
    for (pre, enc), members in by_dims.items():
        rows = np.zeros((len(members), enc), np.uint64)
        for k, i in enumerate(members):
            rows[k, :pre] = vectors[i].reshape(-1)
        coded = LigeroEncoding.new_from_dims(FT63, pre, enc).encode_rows(rows)
        for k, i in enumerate(members):
            results[i] = coded[k].reshape(enc, 1).copy()
    out = []
    for i, (fh, _, columns) in enumerate(reqs):
        opened = fh.read_full_columns(columns)
        if opened:  # one conversion per request: its columns all have the file's row count
            mont = field_to_montgomery(np.stack([np.asarray(c.col).reshape(-1) for c in opened]))
            opened = [LcColumn(mont[k].reshape(-1, 1), c.path) for k, c in enumerate(opened)]
        out.append((results[i], opened))
    return out
