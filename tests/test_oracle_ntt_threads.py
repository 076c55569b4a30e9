"""The oracle's NTT (oracle/of_ntt.c) splits each stage's butterflies over of_set_threads threads.
Field arithmetic is exact and the butterflies of one stage touch disjoint pairs, so the thread
count must not change an output bit: fft_io and ifft_oi on one thread are compared with 2, 3 and
16 threads (three make the ranges uneven; a stage is split down to 2048 butterflies per thread, so
the short rows also pin the unsplit path, 2^13 the first split and 2^16 all sixteen threads).

CPU only: no GPU, no product library."""
import numpy as np
import pytest

FIELDS = {"Ft63": 0, "Ft127": 1, "Ft191": 2, "Ft255": 3, "Ft253_192": 4}
THREADS = (2, 3, 16)
LOGS = tuple(range(1, 15)) + (16,)


@pytest.fixture()
def threads(oracle):
    """set the oracle's thread count; the previous one is restored afterwards"""
    lib = oracle.lib()
    prev = lib.of_get_threads()
    yield lib.of_set_threads
    lib.of_set_threads(prev)


def _rows(oracle, fid, n, seed):
    """a random row and a row of p - 1 (raw Montgomery words: the largest residue)"""
    nl = oracle.limbs(fid)
    pm1 = oracle.limbs_from_ints([oracle.modulus(fid) - 1], nl)
    return {"random": oracle.random_coeffs(fid, n, seed_u64=seed),
            "p-1": np.ascontiguousarray(np.tile(pm1, n))}


def _check(oracle, threads, fid, log_n, seed, kinds=("random", "p-1")):
    n = 1 << log_n
    rows = _rows(oracle, fid, n, seed)
    for name in kinds:
        x = rows[name]
        threads(1)
        fwd = oracle.fft_io(fid, x)
        assert np.array_equal(oracle.ifft_oi(fid, fwd), x), f"{name}: ifft_oi(fft_io(x)) != x"
        for t in THREADS:
            threads(t)
            assert np.array_equal(oracle.fft_io(fid, x), fwd), f"{name}: fft_io differs on {t} threads"
            # (the one-thread ifft_oi of fwd is x, as just shown)
            assert np.array_equal(oracle.ifft_oi(fid, fwd), x), f"{name}: ifft_oi differs on {t} threads"


@pytest.mark.parametrize("field", list(FIELDS))
def test_ntt_thread_count_changes_no_bit(oracle, threads, field):
    fid = FIELDS[field]
    for log_n in LOGS:
        _check(oracle, threads, fid, log_n, seed=0x77EAD000 + 64 * fid + log_n)


def test_ntt_thread_count_changes_no_bit_ft63_2p20(oracle, threads):
    """every thread takes many ranges' worth of butterflies in every one of the twenty stages"""
    _check(oracle, threads, FIELDS["Ft63"], 20, seed=0x77EAD999, kinds=("random",))


def test_get_threads_follows_set_threads(oracle, threads):
    lib = oracle.lib()
    threads(5)
    assert lib.of_get_threads() == 5
    threads(0)  # below one counts as one
    assert lib.of_get_threads() == 1


def test_rows_in_parallel_encode_as_single_rows(oracle, threads):
    """the row-parallel encode calls the NTT from inside a split loop, where the stages run inline:
    every row equals the same row encoded alone (on one thread and on sixteen)"""
    fid, np_, nc, rows = FIELDS["Ft127"], 1 << 13, 1 << 14, 5
    nl = oracle.limbs(fid)
    src = oracle.random_coeffs(fid, rows * np_, seed_u64=0x77EADAAA).reshape(rows, np_ * nl)
    enc = oracle.Encoding.ligero(fid, np_, nc)
    threads(1)
    want = []
    for r in range(rows):
        row = np.zeros(nc * nl, np.uint64)
        row[: np_ * nl] = src[r]
        want.append(oracle.fft_io(fid, row))
    for t in (1, 3, 16):
        threads(t)
        got = enc.encode_rows(src, rows).reshape(rows, nc * nl)
        for r in range(rows):
            assert np.array_equal(got[r], want[r]), f"row {r} on {t} threads"
