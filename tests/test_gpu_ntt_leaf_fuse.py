"""The encode's second pass that also hashes the column leaves (ntt_v2.hpp k_pass_b_leaf, taken by
LcCommit.commit_device for whole-row BLAKE3 commitments of Ft127 encodings whose pass B is 2^8 points
long) against the same commitment made with the separate leaf pass (an encoding created under
LCPC_NTT_LEAF_FUSE=0) and against the CPU oracle.

What can go wrong in the fused pass is the row count, not the row length: a workgroup walks one
1-KiB BLAKE3 chunk of 256 columns' leaf messages (32 zero bytes, then 16 bytes per row) in tiles of
8 rows from row 64 k - 2 on, so the cases are the row counts at which the zero prefix, the tile edges
and the chunk edges fall differently.  Every case commits prefixes of one coefficient matrix that is
uploaded once.

The suite also runs on a build without the kernel (-DLCPC_NTT_LEAF_FUSE=0), where every commitment
takes the separate pass and the same equalities hold; LCPC_NTT_LEAF_FUSE_BUILD=0 in the environment
tells this file that it is looking at such a build (otherwise an encoding that does not fuse fails)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FT63, FT127, FT255 = 0, 1, 3
NP, NC = 1 << 15, 1 << 16
# 1, 2, 3: one partial block, the zero prefix shares the tile; 6, 7: the first tile ends / wraps;
# 61, 62: one chunk, one row short / full (ROOT set in the kernel); 63: a second chunk of one 16-byte
# block; 66, 70: a short second chunk ending inside a tile; 126, 127, 130: a chunk boundary on and one
# row past a tile edge, then a third chunk
ROWS = [1, 2, 3, 6, 7, 61, 62, 63, 66, 70, 126, 127, 130]
MAX_ROWS = max(ROWS)
KERNEL_BUILT = os.environ.get("LCPC_NTT_LEAF_FUSE_BUILD", "1") != "0"


def _encoding(gpu, fid, n_per_row, n_cols, fuse):
    """An encoding made with the environment switch set (fuse False) or absent (True)."""
    old = os.environ.pop("LCPC_NTT_LEAF_FUSE", None)
    try:
        if not fuse:
            os.environ["LCPC_NTT_LEAF_FUSE"] = "0"
        return gpu.RsEncoding.new(fid, n_per_row, n_cols, 4, 1)
    finally:
        os.environ.pop("LCPC_NTT_LEAF_FUSE", None)
        if old is not None:
            os.environ["LCPC_NTT_LEAF_FUSE"] = old


@pytest.fixture(scope="module")
def encs(gpu):
    fused, plain = _encoding(gpu, FT127, NP, NC, True), _encoding(gpu, FT127, NP, NC, False)
    assert not plain.leaf_fuse, "LCPC_NTT_LEAF_FUSE=0 at creation must keep the separate leaf pass"
    assert fused.leaf_fuse == KERNEL_BUILT
    return fused, plain


@pytest.fixture(scope="module")
def matrix(oracle, hipmem):
    """MAX_ROWS rows of coefficients, on the host and on the device (read only)."""
    coeffs = oracle.ChaCha(seed_u64=0x1EAF).field_random(FT127, MAX_ROWS * NP)
    d = hipmem.to_device(coeffs)
    yield coeffs, d
    hipmem.free(d)


def _commit(gpu, d, length, enc):
    """(commitment, the names of the kernels it launched)"""
    gpu.prof_enable(True)
    gpu.prof_reset()
    try:
        c = gpu.LcCommit.commit_device(d, length, enc)
        return c, set(gpu.prof_stats())
    finally:
        gpu.prof_enable(False)


def _check_pair(gpu, oracle, fid, d, length, fused, plain, n_cols, expect_fused):
    """The commitment of d[:length] under `fused` equals the one under `plain` bit for bit, took the
    expected path, and its leaf layer is the oracle's BLAKE3 of the downloaded codeword."""
    g, ran = _commit(gpu, d, length, fused)
    h, ran_plain = _commit(gpu, d, length, plain)
    assert "leaf_chunks" in ran_plain and "ntt_pass_b" in ran_plain
    assert ("leaf_chunks" not in ran) == expect_fused, sorted(ran)
    assert "ntt_pass_b" in ran
    n_rows = g.get_n_rows()
    comm = g.comm
    assert np.array_equal(comm, h.comm)
    assert np.array_equal(g.coeffs, h.coeffs)
    hashes = g.hashes
    assert hashes == h.hashes  # leaf layer, every level above it, the root
    assert g.get_root() == h.get_root() == hashes[-32:]
    assert hashes[:32 * n_cols] == oracle.hash_columns(fid, comm.reshape(-1), n_rows, n_cols)
    return g, h


@pytest.mark.parametrize("n_rows", ROWS)
def test_fused_commit_matches_separate_pass(gpu, oracle, encs, matrix, n_rows):
    fused, plain = encs
    coeffs, d = matrix
    g, _ = _check_pair(gpu, oracle, FT127, d, n_rows * NP, fused, plain, NC, fused.leaf_fuse)
    assert g.get_n_rows() == n_rows
    if n_rows <= 7:  # the oracle's own commit (its FFTs, its tree)
        nl = oracle.limbs(FT127)
        o = oracle.Commit(oracle.Encoding.ligero(FT127, NP, NC, 4, 1), coeffs[:n_rows * NP * nl])
        assert g.get_root() == o.root()
        assert g.hashes == o.hashes


@pytest.mark.parametrize("n_rows", [3, 63, 127])
def test_fused_commit_half_as_many_columns(gpu, oracle, matrix, n_rows):
    """n_cols = 2^15 is the other row length whose pass B is 2^8 points long: the same kernel over
    128 column blocks instead of 256 (the matrix's leading coefficients, re-cut into shorter rows)."""
    np_, nc = NP // 2, NC // 2
    fused, plain = _encoding(gpu, FT127, np_, nc, True), _encoding(gpu, FT127, np_, nc, False)
    assert fused.leaf_fuse == KERNEL_BUILT and not plain.leaf_fuse
    coeffs, d = matrix
    g, _ = _check_pair(gpu, oracle, FT127, d, n_rows * np_, fused, plain, nc, fused.leaf_fuse)
    assert g.get_n_rows() == n_rows
    if n_rows <= 7:
        o = oracle.Commit(oracle.Encoding.ligero(FT127, np_, nc, 4, 1), coeffs[:n_rows * np_ * oracle.limbs(FT127)])
        assert g.hashes == o.hashes


def test_ragged_length_takes_the_separate_pass(gpu, oracle, encs, matrix):
    """A last row that is not whole: the fused entry needs every row in one call, so the commitment
    keeps the two kernels under either encoding."""
    fused, plain = encs
    coeffs, d = matrix
    length = 5 * NP + 77
    g, _ = _check_pair(gpu, oracle, FT127, d, length, fused, plain, NC, False)
    assert g.get_n_rows() == 6
    nl = oracle.limbs(FT127)
    o = oracle.Commit(oracle.Encoding.ligero(FT127, NP, NC, 4, 1), coeffs[:length * nl])
    assert g.get_root() == o.root()


def test_prove_and_verify_70_rows(gpu, oracle, encs, matrix):
    fused, plain = encs
    _, d = matrix
    n_rows, nco = 70, fused.get_n_col_opens()
    g = gpu.LcCommit.commit_device(d, n_rows * NP, fused)
    h = gpu.LcCommit.commit_device(d, n_rows * NP, plain)
    root = g.get_root()
    x = oracle.ChaCha(seed_u64=70).field_random(FT127, 1)
    inner, outer = oracle.eval_tensors(FT127, x, NP, n_rows)

    def tr():
        t = gpu.Transcript(b"test transcript")
        t.append_message(b"polycommit", root)
        t.append_message(b"ncols", nco.to_bytes(8, "big"))
        return t

    pf, ph = g.prove(outer, fused, tr()), h.prove(outer, plain, tr())
    assert np.array_equal(pf.p_eval, ph.p_eval)
    for a, b in zip(pf.columns, ph.columns):
        assert np.array_equal(a.col, b.col) and a.path == b.path
    ev = pf.verify(root, outer, inner, fused, tr())
    assert np.array_equal(ev, ph.verify(root, outer, inner, plain, tr()))


@pytest.mark.parametrize("fid", [FT63, FT255])
def test_other_fields_keep_the_separate_pass(gpu, oracle, hipmem, fid):
    """The same row length in a field the kernel is not built for: the switch changes nothing."""
    on, off = _encoding(gpu, fid, NP, NC, True), _encoding(gpu, fid, NP, NC, False)
    assert not on.leaf_fuse and not off.leaf_fuse
    n_rows = 3
    coeffs = oracle.ChaCha(seed_u64=0xF1D + fid).field_random(fid, n_rows * NP)
    d = hipmem.to_device(coeffs)
    try:
        g, _ = _check_pair(gpu, oracle, fid, d, n_rows * NP, on, off, NC, False)
        o = oracle.Commit(oracle.Encoding.ligero(fid, NP, NC, 4, 1), coeffs)
        assert g.get_root() == o.root()
    finally:
        hipmem.free(d)
