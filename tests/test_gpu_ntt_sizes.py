"""GPU: the four-step NTT at every row length it dispatches, 2^17 .. 2^24 (2^22 for the 32-byte
fields), against the oracle's fft_io -- whole rows, np.array_equal, no tolerance.

ntt_rows_t (csrc/ntt_impl.hpp) instantiates k_pass_a for the sub-transform length L = l1 and
k_pass_b for L = l2 (ntt_plan_init: l1 = log_n // 2, l2 = log_n - l1), pass A further in the four
HALFZ x CANON variants.  The rest of the suite stops at 2^16 (plus one Ft127 commit at 2^20), so
it launches L in {6, 7, 8} only.  The lengths here launch the others:

    log_n   l1  l2      fields
    17       8   9      all
    18       9   9      all
    19       9  10      all
    20      10  10      all
    21      10  11      all
    22      11  11      all      (the top for Ft191, Ft255, Ft253_192: HI = 11)
    23      11  12      Ft63, Ft127
    24      12  12      Ft63, Ft127   (HI = 12)

    (13: 6/7, 14: 7/7, 15: 7/8 -- Ft63: 8/7 -- and 16: 8/8 are test_gpu_parity.py's; the four
    pass-A variants at those lengths are test_selftest_entry_at_the_lengths_other_tests_trust's.)

so pass A runs at L = 8..12 (8..11) and pass B at L = 9..12 (9..11) for every field, pass A in all
four variants (below).  What changes with L: the tile width CW = 2^(E - L) shrinks to 4, 2, 1
columns (E = 12, 11, 10 for Ft63, Ft127, the wide fields), the LDS row pitch LD = CW + 1 becomes 1 at CW = 1, log_cw() clamps to 0 for L > E (one
workgroup then owns a vector larger than the tuned tile, up to 96 KiB of static LDS), and the
chain of lazy [0, 2p) butterflies between two reductions is at its longest.

Each case has one row and one reference.  n_valid = n/2 is the rate-1/2 row (HALFZ: the upper
half is never loaded); n_valid = n/2 + 1 is the first length that leaves that path and needs the
general path's `pos < n_valid` padding.  lcpc_selftest_ntt_rows calls ntt_rows with the caller's
n_valid, strides, copy buffer and canon flag; the public lcpc_encode / lcpc_encode_rows upload
the whole zero-padded row and transform it in place, i.e. with n_valid = n -- so they pin the
general path on the same row, and HALFZ is pinned by the selftest calls.  lcpc_ifft_oi_rows on the
reference gives the row back: the inverse-root tables, the general passes and both k_bitrev_scale
launches at the same length.

The references come from the oracle on min(16, CPUs of this process) threads (oracle/of_ntt.c:
the thread count changes no bit, tests/test_oracle_ntt_threads.py)."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELD_NAMES = {0: "Ft63", 1: "Ft127", 2: "Ft191", 3: "Ft255", 4: "Ft253_192"}
MAX_LOG_N = {0: 24, 1: 24, 2: 22, 3: 22, 4: 22}  # ntt_max_log_n (csrc/ntt.hip)
UNSUPPORTED = 34  # LCPC_ERR_UNSUPPORTED
SENTINEL = np.uint64(0xA5C3A5C3A5C3A5C3)

SIZE_CASES = [pytest.param(fid, log_n, halfz, id=f"{FIELD_NAMES[fid]}-2p{log_n}-{'halfz' if halfz else 'general'}")
              for fid in FIELD_NAMES for log_n in range(17, MAX_LOG_N[fid] + 1) for halfz in (True, False)]


@pytest.fixture(scope="module", autouse=True)
def oracle_threads(oracle):
    lib = oracle.lib()
    prev = lib.of_get_threads()
    lib.of_set_threads(min(16, len(os.sched_getaffinity(0))))
    yield
    lib.of_set_threads(prev)


def _canonical(oracle, fid, a):
    out = np.zeros_like(a)
    oracle.lib().of_to_canonical(fid, oracle.p64(a), oracle.p64(out), a.size // oracle.limbs(fid))
    return out


def _padded_row(oracle, fid, n, nv, seed):
    row = np.zeros(n * oracle.limbs(fid), np.uint64)
    row[: nv * oracle.limbs(fid)] = oracle.random_coeffs(fid, nv, seed_u64=seed)
    return row


def _selftest_both_forms(gpu, fid, log_n, row, nv, want, want_canon, label):
    """ntt_rows on one row through the selftest entry, Montgomery and canonical output, with the
    fused coefficient copy.  src carries the sentinel beyond n_valid (it must read as zero), copy
    is a whole row long (beyond n_valid it must keep the sentinel)."""
    n, nl = 1 << log_n, row.size >> log_n
    src = row.copy()
    src[nv * nl:] = SENTINEL
    for canon, ref in ((False, want), (True, want_canon)):
        dst = np.full(n * nl, SENTINEL, np.uint64)
        cp = np.full(n * nl, SENTINEL, np.uint64)
        gpu.selftest_ntt_rows(fid, log_n, src, nv, dst, src_stride=n, copy=cp, copy_stride=n, canon=canon)
        assert np.array_equal(dst, ref), f"{label}: ntt_rows, canon={canon}"
        assert np.array_equal(cp[: nv * nl], row[: nv * nl]), f"{label}: coefficient copy, canon={canon}"
        assert (cp[nv * nl:] == SENTINEL).all(), f"{label}: copy written beyond n_valid, canon={canon}"
        del dst, cp


@pytest.mark.parametrize("fid,log_n,halfz", SIZE_CASES)
def test_every_dispatched_length(gpu, oracle, fid, log_n, halfz):
    from lcpc_proof_of_storage_amd import pos
    n, nl = 1 << log_n, oracle.limbs(fid)
    nv = n // 2 if halfz else n // 2 + 1
    label = f"{FIELD_NAMES[fid]} 2^{log_n} n_valid={nv}"
    t0 = time.perf_counter()
    row = _padded_row(oracle, fid, n, nv, seed=0x5170000 + 1000 * fid + 2 * log_n + halfz)
    want = oracle.fft_io(fid, row)
    want_canon = _canonical(oracle, fid, want)
    t1 = time.perf_counter()

    # the public encode of the zero-padded row (one row: lcpc_encode; lcpc_encode_rows for the other)
    enc = gpu.RsEncoding.new(fid, n // 2, n, 4, 1)
    got = row.copy()
    if halfz:
        enc.encode(got)
    else:
        got = enc.encode_rows(got.reshape(1, -1)).reshape(-1)
    del enc  # (frees the plan's four tables before the next one is made)
    assert np.array_equal(got, want), f"{label}: public encode"
    del got

    _selftest_both_forms(gpu, fid, log_n, row, nv, want, want_canon, label)

    back = pos.ifft_oi_rows(want.reshape(1, n, nl), fid).reshape(-1)
    assert np.array_equal(back, row), f"{label}: ifft_oi of the reference"
    t2 = time.perf_counter()
    print(f"\n[ntt_sizes] {label}: reference {t1 - t0:.2f} s, GPU calls and compares {t2 - t1:.2f} s")


@pytest.mark.parametrize("fid", list(FIELD_NAMES), ids=list(FIELD_NAMES.values()))
def test_extremes_at_the_deepest_transform(gpu, oracle, fid):
    """A full-length row of p - 1 (raw Montgomery words) at the field's longest row: every sum and
    difference of the longest chain of lazy [0, 2p) butterflies sits at its carry / borrow
    boundary."""
    log_n = MAX_LOG_N[fid]
    n, nl = 1 << log_n, oracle.limbs(fid)
    pm1 = oracle.limbs_from_ints([oracle.modulus(fid) - 1], nl)
    row = np.ascontiguousarray(np.tile(pm1, n))
    want = oracle.fft_io(fid, row)
    _selftest_both_forms(gpu, fid, log_n, row, n, want, _canonical(oracle, fid, want),
                         f"{FIELD_NAMES[fid]} 2^{log_n} all p-1")


@pytest.mark.parametrize("fid", list(FIELD_NAMES), ids=list(FIELD_NAMES.values()))
def test_strides_and_rows_at_2p18(gpu, oracle, fid):
    """Three rows with every stride above its row length (the commit paths only pass
    src_stride = n_per_row, dst_stride = n_cols): each row equals its own reference and the gap
    elements of dst and copy keep the sentinel."""
    log_n, rows = 18, 3
    n, nl = 1 << log_n, oracle.limbs(fid)
    nv = n // 2 - 3
    ss, ds, cs = nv + 5, n + 7, nv + 1
    coeffs = oracle.random_coeffs(fid, rows * nv, seed_u64=0x5172000 + fid).reshape(rows, nv * nl)
    src = np.full((rows, ss * nl), SENTINEL, np.uint64)
    src[:, : nv * nl] = coeffs
    want = []
    for r in range(rows):
        row = np.zeros(n * nl, np.uint64)
        row[: nv * nl] = coeffs[r]
        want.append(oracle.fft_io(fid, row))
    for canon in (False, True):
        dst = np.full((rows, ds * nl), SENTINEL, np.uint64)
        cp = np.full((rows, cs * nl), SENTINEL, np.uint64)
        gpu.selftest_ntt_rows(fid, log_n, src, nv, dst, n_rows=rows, src_stride=ss, dst_stride=ds, copy=cp,
                              copy_stride=cs, canon=canon)
        for r in range(rows):
            ref = _canonical(oracle, fid, want[r]) if canon else want[r]
            assert np.array_equal(dst[r, : n * nl], ref), f"row {r}, canon={canon}"
            assert np.array_equal(cp[r, : nv * nl], coeffs[r]), f"copy of row {r}, canon={canon}"
        assert (dst[:, n * nl:] == SENTINEL).all(), f"dst gap written, canon={canon}"
        assert (cp[:, nv * nl:] == SENTINEL).all(), f"copy gap written, canon={canon}"


def _bitrev_index(log_n):
    idx = np.arange(1 << log_n, dtype=np.int64)
    rev = np.zeros_like(idx)
    for b in range(log_n):
        rev |= ((idx >> b) & 1) << (log_n - 1 - b)
    return rev


@pytest.mark.parametrize("fid", list(FIELD_NAMES), ids=list(FIELD_NAMES.values()))
def test_inverse_plan_through_the_selftest_entry(gpu, oracle, fid):
    """inverse = 1: the DIF with the inverse root, never reordered, never scaled --
    y[bitrev(i)] = sum_j x[j] w^(-i j) -- which is n * ifft_oi's output at i when ifft_oi is fed x
    as the evaluations (in the order the oracle's convention reads them).  2^13 is the first
    four-step length, 2^18 runs both passes at L = 9; n_valid = n is the only length the inverse
    plans are ever called with."""
    nl = oracle.limbs(fid)
    # the oracle's output order (include/lcpc_fft_convention.h): fft_io of (0, 1, 0, 0) is
    # (1, w, w^2, w^3) in natural order and (1, w^2, w, w^3) bit-reversed
    w4 = np.zeros(nl, np.uint64)
    oracle.lib().of_ntt_omega(fid, 2, oracle.p64(w4))
    probe = oracle.fft_io(fid, oracle.to_mont(fid, [0, 1, 0, 0])).reshape(4, nl)
    evals_bitrev = not np.array_equal(probe[1], w4)
    for log_n in (13, 18):
        n = 1 << log_n
        rev = _bitrev_index(log_n)
        x = oracle.random_coeffs(fid, n, seed_u64=0x5174000 + 100 * fid + log_n).reshape(n, nl)
        z = np.ascontiguousarray(x[rev] if evals_bitrev else x)  # z[bitrev(j)] = x[j]
        scaled = oracle.mul(fid, oracle.ifft_oi(fid, z.reshape(-1)), np.tile(oracle.to_mont(fid, [n]), n))
        want = np.ascontiguousarray(scaled.reshape(n, nl)[rev]).reshape(-1)  # want[bitrev(i)] = n ifft_oi(z)[i]
        dst = np.full(n * nl, SENTINEL, np.uint64)
        gpu.selftest_ntt_rows(fid, log_n, np.ascontiguousarray(x.reshape(-1)), n, dst, inverse=True)
        assert np.array_equal(dst, want), f"{FIELD_NAMES[fid]} 2^{log_n}"


@pytest.mark.parametrize("fid", list(FIELD_NAMES), ids=list(FIELD_NAMES.values()))
def test_selftest_entry_at_the_lengths_other_tests_trust(gpu, oracle, fid):
    """The entry itself where the public encode is already pinned (length 1, the whole-row-in-LDS
    kernel up to 2^12, the first four-step lengths, Ft63's l1 = 8 split at 2^15): both halves of
    the HALFZ threshold, Montgomery and canonical output, the copy -- the pass-A variants that
    only the commit paths reach otherwise."""
    for log_n in (0, 1, 5, 12, 13, 14, 15, 16):
        n = 1 << log_n
        for nv in sorted({max(n // 2, 1), min(n // 2 + 1, n), n}):
            row = _padded_row(oracle, fid, n, nv, seed=0x5173000 + 100 * fid + log_n)
            want = oracle.fft_io(fid, row)
            _selftest_both_forms(gpu, fid, log_n, row, nv, want, _canonical(oracle, fid, want),
                                 f"{FIELD_NAMES[fid]} 2^{log_n} n_valid={nv}")


@pytest.mark.parametrize("fid", list(FIELD_NAMES), ids=list(FIELD_NAMES.values()))
def test_one_past_the_range_is_refused(gpu, oracle, fid):
    """2^(max + 1) points: the encoding, ifft_oi and the selftest entry all answer
    LCPC_ERR_UNSUPPORTED (the plan refuses before it allocates its tables); 2^max itself succeeds
    in test_every_dispatched_length."""
    from lcpc_proof_of_storage_amd import pos
    log_n = MAX_LOG_N[fid] + 1
    n, nl = 1 << log_n, oracle.limbs(fid)
    with pytest.raises(gpu.LcpcError) as e:
        gpu.RsEncoding.new(fid, 1, n, 4, 1)
    assert e.value.code == UNSUPPORTED
    big = np.zeros((1, n, nl), np.uint64)  # (never touched: untouched zero pages)
    with pytest.raises(gpu.LcpcError) as e:
        pos.ifft_oi_rows(big, fid)
    assert e.value.code == UNSUPPORTED
    for inverse in (False, True):
        with pytest.raises(gpu.LcpcError) as e:
            gpu.selftest_ntt_rows(fid, log_n, big.reshape(-1), n, big.reshape(-1), inverse=inverse)
        assert e.value.code == UNSUPPORTED
