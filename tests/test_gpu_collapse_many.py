"""GPU: the many-tensor row combination (lcpc_collapse_columns_many, csrc/collapse.hip) against the
oracle's collapse called once per tensor, word for word.  The tensor counts sit around the kernel's
chunk size (lcpc_collapse_many_chunk: tensors per thread and pass over the coefficients), the row
counts around the 16-row split granule, the 512-row bound of the int8 accumulators and one row, the
column counts around the 64-lane wave and the 256-thread block.  Inputs are random elements, the
extremes (p - 1 everywhere; 0 alternating with p - 1) and, for Ft127 at 512 and 513 rows, the
digit-aligned coefficients of test_gpu_collapse.py, which drive int8 accumulators toward 2^27."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_TENSORS = [1, 4, 5, 7, 8, 9, 16, 17, 33, 65]
ROWS_FT127 = [1, 3, 4, 5, 15, 16, 17, 511, 512, 513, 1025]
ROWS_OTHER = [1, 5, 17, 513]
PER_ROW = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257]


def _chunk_sizes():
    """the kernel's tensors per chunk for every field, from the library (a host-only call)"""
    from lcpc_proof_of_storage_amd import _native as N
    return {f: N.load().lcpc_collapse_many_chunk(f) for f in range(5)}


CHUNK = _chunk_sizes()


def _tensor_counts(fid):
    tt = CHUNK[fid]
    return sorted(set(N_TENSORS + [max(tt - 1, 1), tt, tt + 1, 2 * tt + 1]))


def _cases():
    """a covering set: every value of every dimension in at least one Ft127 case, the other fields
    on their four row counts"""
    out = []
    nts = _tensor_counts(1)
    for i in range(max(len(nts), len(ROWS_FT127), len(PER_ROW)) + 11):
        out.append((1, nts[i % len(nts)], ROWS_FT127[(i * 3) % len(ROWS_FT127)], PER_ROW[(i * 7) % len(PER_ROW)]))
    for fid in (0, 2, 3, 4):
        nts = _tensor_counts(fid)
        for i in range(9):
            out.append((fid, nts[(i * 5 + fid) % len(nts)], ROWS_OTHER[i % 4], PER_ROW[(i * 3 + fid) % len(PER_ROW)]))
    return out


CASES = _cases()


def test_case_table_covers_every_value():
    ft127 = [c for c in CASES if c[0] == 1]
    assert {c[1] for c in ft127} >= set(_tensor_counts(1))
    assert {c[2] for c in ft127} == set(ROWS_FT127)
    assert {c[3] for c in ft127} == set(PER_ROW)
    for fid in (0, 2, 3, 4):
        assert {c[2] for c in CASES if c[0] == fid} == set(ROWS_OTHER)
    assert 55 <= len(CASES) <= 70


def test_chunk_sizes_are_the_librarys(gpu):
    assert all(1 <= CHUNK[f] <= 64 for f in range(5)), CHUNK
    assert gpu.collapse_many_chunk(5) == 0
    assert gpu.BATCH_MAX_TENSORS >= 1024


def _check(gpu, oracle, fid, coeffs, tens, n_rows, n_per_row):
    got = gpu.collapse_columns_many(fid, coeffs, tens, n_rows, n_per_row)
    assert got.shape[:2] == (tens.shape[0], n_per_row)
    for t in range(tens.shape[0]):
        want = oracle.collapse(fid, coeffs.reshape(-1), tens[t].reshape(-1), n_rows, n_per_row)
        assert np.array_equal(got[t].reshape(-1), want), f"tensor {t}"
    return got


@pytest.mark.parametrize("fid,n_t,n_rows,n_per_row", CASES)
def test_random_inputs_match_oracle(gpu, oracle, fid, n_t, n_rows, n_per_row):
    rng = oracle.ChaCha(seed_u64=fid * 100003 + n_t * 1009 + n_rows * 31 + n_per_row)
    coeffs = rng.field_random(fid, n_rows * n_per_row)
    tens = rng.field_random(fid, n_t * n_rows).reshape(n_t, n_rows, -1)
    got = _check(gpu, oracle, fid, coeffs, tens, n_rows, n_per_row)
    if n_t <= 4:  # the same call per tensor through the 1-4 tensor entry
        for t in range(n_t):
            assert np.array_equal(got[t], gpu.collapse_columns(fid, coeffs, tens[t], n_rows, n_per_row))


@pytest.mark.parametrize("pattern", ["max", "alternating"])
@pytest.mark.parametrize("fid,n_t,n_rows,n_per_row", [(1, 9, 513, 65), (1, 17, 512, 17), (0, 17, 17, 65),
                                                      (2, 6, 513, 15), (3, 5, 17, 257), (4, 9, 5, 64)])
def test_extremes_match_oracle(gpu, oracle, fid, n_t, n_rows, n_per_row, pattern):
    import field_ref as FR
    fr = FR.field_ref(fid)
    top = fr.p - 1
    grid = [[top if pattern == "max" or (r + c) % 2 else 0 for c in range(n_per_row)] for r in range(n_rows)]
    coeffs = fr.to_array([v for row in grid for v in row]).reshape(-1)
    tens = np.tile(fr.to_array([top]), (n_t, n_rows, 1))
    got = _check(gpu, oracle, fid, coeffs, tens, n_rows, n_per_row)
    count = [sum(1 for r in range(n_rows) if grid[r][c]) for c in range(n_per_row)]
    want = [k * top * top * fr.Rinv % fr.p for k in count]
    for t in range(n_t):
        assert fr.from_array(got[t]) == want, f"tensor {t}"


# ---- digit-aligned adversarial inputs (test_gpu_collapse.py's construction, rebuilt here): every
# row of tensor t holds one word T_t, every row of a column one coefficient whose balanced digits
# d_a are 127 where the digit h[a][u] of T_t 2^(8a) mod p has the targeted sign and -128 elsewhere,
# so an int8 accumulator Y_u of that (tensor, column) grows by about 2^17 per row.
ADV_T = 9
ADV_TARGETS = [(u, s) for u in (0, 7, 14, 15) for s in (1, -1)]
ADV_PER_ROW = (1 << 26) // 512


def _adv_per_row(fr, T):
    """the least |Y_u| growth per row over the targets for tensor word T, in the test's integer model"""
    import field_ref as FR
    h = [FR.balanced_digits((T << (8 * a)) % fr.p) for a in range(16)]
    worst = None
    for u, s in ADV_TARGETS:
        d = FR.balanced_digits(_adv_coefficient(fr, h, u, s))
        y = sum(h[a][u] * d[a] for a in range(16)) * s
        worst = y if worst is None else min(worst, y)
    return worst


def _adv_tensor_words(fr):
    """ADV_T words from a fixed-seed search: the 100 candidates with the largest digit mass at the
    targeted positions, of those the ADV_T whose coefficients grow an accumulator fastest"""
    import random
    rng = random.Random(0xADC1)
    cands = [rng.randrange(fr.p) for _ in range(20000)]
    off = int.from_bytes(b"\x80" * 16, "little")
    us = sorted({u for u, _ in ADV_TARGETS})

    def score(T):
        tot = [0] * 16
        for a in range(16):
            for u, byte in enumerate((((T << (8 * a)) % fr.p) + off).to_bytes(16, "little")):
                tot[u] += abs(byte - 128)
        return min(tot[u] for u in us)
    top = sorted(cands, key=score, reverse=True)[:100]
    return sorted(top, key=lambda T: _adv_per_row(fr, T), reverse=True)[:ADV_T]


def _adv_coefficient(fr, h, u, s):
    d = [127 if h[a][u] * s > 0 else -128 for a in range(15)]
    low = sum(v << (8 * a) for a, v in enumerate(d))
    d15_min = 0 if low >= 0 else 1
    d15_max = min((fr.p - 1 - low) >> 120, 127)
    x = low + ((d15_max if h[15][u] * s > 0 else d15_min) << 120)
    assert 0 <= x < fr.p
    return x


@pytest.fixture(scope="module")
def adversarial():
    import field_ref as FR
    fr = FR.field_ref(1)
    Ts = _adv_tensor_words(fr)
    hs = [[FR.balanced_digits((T << (8 * a)) % fr.p) for a in range(16)] for T in Ts]
    n_per_row = 72
    xs = []
    for c in range(n_per_row):
        t = c % ADV_T
        u, s = ADV_TARGETS[(c // ADV_T) % len(ADV_TARGETS)]
        x = _adv_coefficient(fr, hs[t], u, s)
        d = FR.balanced_digits(x)
        assert sum(hs[t][a][u] * d[a] for a in range(16)) * s >= ADV_PER_ROW
        xs.append(x)
    return fr, Ts, xs


@pytest.mark.parametrize("n_rows", [512, 513])
def test_ft127_adversarial_digits(gpu, oracle, adversarial, n_rows):
    fr, Ts, xs = adversarial
    coeffs = np.tile(fr.to_array(xs).reshape(1, -1), (n_rows, 1)).reshape(-1)
    tens = np.stack([np.tile(fr.to_array([T]), (n_rows, 1)) for T in Ts])
    got = _check(gpu, oracle, 1, coeffs, tens, n_rows, len(xs))
    for t, T in enumerate(Ts):
        assert fr.from_array(got[t]) == [n_rows * T * x * fr.Rinv % fr.p for x in xs], f"tensor {t}"


def test_valu_only_child_gives_the_same_bytes(gpu, tmp_path):
    """LCPC_NO_MFMA=1 is read once per process: a child recomputes six Ft127 cases under it"""
    import _collapse_many_child as child
    here = child.run_cases()
    out = tmp_path / "child.bin"
    env = dict(os.environ, LCPC_NO_MFMA="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_collapse_many_child.py"), str(out)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == here
    assert len(here) == sum(n_t * n_per_row * 16 for n_t, _, n_per_row in child.CHILD_CASES)


def test_tensor_count_bounds(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    lib = N.load()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data_as(N.u64p)
    assert lib.lcpc_collapse_columns_many(1, p, 2, 2, p, 0, p) == 30
    assert lib.lcpc_collapse_columns_many(1, p, 2, 2, p, gpu.BATCH_MAX_TENSORS + 1, p) == 30
    assert "n_tensors" in N.last_error()
    assert lib.lcpc_collapse_columns_many(7, p, 2, 2, p, 1, p) == 30
