"""GPU: the Ft127 encode passes on word-expanded twiddles (csrc/ntt_v2.hpp, TwWords; fe_mul_tw of
csrc/field.hpp) against the oracle's fft_io, whole rows, np.array_equal.

ntt_rows_t gives the expanded-twiddle policy to every Ft127 pass of at most 2^9 points.  The
lengths below are the smallest that dispatch each of its (L, CW, T) instantiations:

    log_n   pass A (L, CW, T)   pass B (L, CW, T)
    13      (6, 5, 8)           (7, 4, 8)
    14      (7, 5, 10)          (7, 5, 10)     the cfg2 pair
    15      (7, 4, 8)           (8, 3, 8)
    16      (8, 3, 8)           (8, 3, 8)      the flagship's rows
    17      (8, 3, 8)           (9, 2, 8)
    18      (9, 2, 8)           (9, 2, 8)      three rows, every stride above its row length

(2^19 and 2^20 run one or both passes at L = 10, which keeps the one-element twiddles;
tests/test_gpu_ntt_sizes.py has every length from 2^17 to 2^24.)

Per length: three rows; n_valid = n/2 (the half-zero first stage: products only), n/2 + 1 and n;
Montgomery and canonical output with the fused coefficient copy; inputs random, all p - 1,
alternating 0 / p - 1, and a single nonzero element at the last valid position -- all in [0, p), so
the oracle alone defines the result.  Each row equals its reference, the copy equals the input,
and lcpc_ifft_oi_rows (inverse plans run the same kernels on the same kind of table) takes the
reference back to the input.  One commit + prove at 2^16 coefficients against the oracle ends the
file.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FID = 1
SENTINEL = np.uint64(0xA5C3A5C3A5C3A5C3)
ROWS = 3
KINDS = ("random", "all_pm1", "alternating", "last_only")


def _canonical(oracle, a):
    out = np.zeros_like(a)
    oracle.lib().of_to_canonical(FID, oracle.p64(a), oracle.p64(out), a.size // oracle.limbs(FID))
    return out


def _inputs(oracle, kind, nv, seed):
    """(ROWS, nv, limbs) raw Montgomery words, every element < p."""
    nl = oracle.limbs(FID)
    pm1 = oracle.limbs_from_ints([oracle.modulus(FID) - 1], nl).reshape(nl)
    if kind == "random":
        return oracle.random_coeffs(FID, ROWS * nv, seed_u64=seed).reshape(ROWS, nv, nl).copy()
    x = np.zeros((ROWS, nv, nl), np.uint64)
    if kind == "all_pm1":
        x[:] = pm1
    elif kind == "alternating":
        for r in range(ROWS):
            x[r, (r & 1)::2] = pm1  # (row 1 starts with p - 1, rows 0 and 2 with 0)
    else:
        x[0, nv - 1] = pm1
        x[1, nv - 1, 0] = 1
        x[2, nv - 1] = oracle.random_coeffs(FID, 1, seed_u64=seed).reshape(nl)
    return x


def _check(gpu, oracle, log_n, nv, kind, ss, ds, cs):
    from lcpc_proof_of_storage_amd import pos
    n, nl = 1 << log_n, oracle.limbs(FID)
    label = f"2^{log_n} n_valid={nv} {kind}"
    x = _inputs(oracle, kind, nv, seed=0x7420000 + 100 * log_n + KINDS.index(kind))
    padded = np.zeros((ROWS, n, nl), np.uint64)
    padded[:, :nv] = x
    want = np.stack([oracle.fft_io(FID, np.ascontiguousarray(padded[r].reshape(-1))) for r in range(ROWS)])
    src = np.full((ROWS, ss * nl), SENTINEL, np.uint64)
    src[:, : nv * nl] = x.reshape(ROWS, -1)
    for canon in (False, True):
        ref = np.stack([_canonical(oracle, want[r]) for r in range(ROWS)]) if canon else want
        dst = np.full((ROWS, ds * nl), SENTINEL, np.uint64)
        cp = np.full((ROWS, cs * nl), SENTINEL, np.uint64)
        gpu.selftest_ntt_rows(FID, log_n, src, nv, dst, n_rows=ROWS, src_stride=ss, dst_stride=ds, copy=cp,
                              copy_stride=cs, canon=canon)
        for r in range(ROWS):
            assert np.array_equal(dst[r, : n * nl], ref[r]), f"{label}: row {r}, canon={canon}"
            assert np.array_equal(cp[r, : nv * nl], x[r].reshape(-1)), f"{label}: copy of row {r}, canon={canon}"
        assert (dst[:, n * nl:] == SENTINEL).all(), f"{label}: dst gap written, canon={canon}"
        assert (cp[:, nv * nl:] == SENTINEL).all(), f"{label}: copy written beyond n_valid, canon={canon}"
    back = pos.ifft_oi_rows(want.reshape(ROWS, n, nl), FID)
    assert np.array_equal(back, padded), f"{label}: ifft_oi of the reference"


@pytest.mark.parametrize("log_n", [13, 14, 15, 16, 17])
def test_every_expanded_twiddle_instantiation(gpu, oracle, log_n):
    n = 1 << log_n
    for nv in (n // 2, n // 2 + 1, n):
        for kind in KINDS:
            _check(gpu, oracle, log_n, nv, kind, ss=nv, ds=n, cs=nv)


def test_strided_rows_at_2p18(gpu, oracle):
    n = 1 << 18
    for nv in (n // 2, n // 2 + 1, n):
        for kind in KINDS:
            _check(gpu, oracle, 18, nv, kind, ss=nv + 5, ds=n + 7, cs=nv + 1)


def test_commit_and_prove_at_2p16_match_the_oracle(gpu, oracle):
    """Ft127, 2^16 coefficients: root, p_eval and the opened columns."""
    L, O = gpu, oracle
    length = 1 << 16
    coeffs = O.random_coeffs(FID, length, seed_u64=0x7421)
    enc = L.LigeroEncoding.new(FID, length)
    comm = L.LcCommit.commit(coeffs, enc)
    o_enc = O.Encoding.ligero_new(FID, length)
    o_comm = O.Commit(o_enc, coeffs)
    assert comm.get_root() == o_comm.root()
    x = O.ChaCha(seed_u64=11).field_random(FID, 1)
    _, outer = O.eval_tensors(FID, x, comm.get_n_per_row(), comm.get_n_rows())
    nco = enc.get_n_col_opens()
    tr = L.Transcript(b"test transcript")
    tr.append_message(b"polycommit", comm.get_root())
    tr.append_message(b"ncols", nco.to_bytes(8, "big"))
    pf = comm.prove(outer, enc, tr)
    op = o_comm.prove(o_enc, outer, O.standard_transcript(nco, o_comm.root()))
    assert np.array_equal(pf.p_eval.reshape(-1), op.p_eval)
    cols = pf.columns
    assert len(cols) == nco
    o_cols = op.cols.reshape(nco, -1)
    o_paths = op.paths.tobytes()
    for k, c in enumerate(cols):
        assert np.array_equal(c.col.reshape(-1), o_cols[k]), f"opened column {k}"
        assert b"".join(c.path) == o_paths[k * 32 * op.path_len:(k + 1) * 32 * op.path_len], f"path {k}"
