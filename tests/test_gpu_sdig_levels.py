"""GPU: one sparse level of the Brakedown encode, y = M x (csrc/sdig.hip), on matrices the test
writes itself (lcpc_selftest_spmm), against Python integers:

    y[j][b] = sum_k val_k x[idx_k][b] R^-1 mod p        (elements as the library stores them)

The encode reaches these kernels only with matgen's matrices (a few dozen nonzeros per output) and
random messages.  Here: every instantiation of the Ft127 matrix-core kernel (1 to 8 tiles of 16
rows, one wave or four per output, one to three row chunks with a partial last one), outputs with
0 to 17 nonzeros next to each other, a strict sub-range of the rows, the int32 digit accumulators
driven to the 512-nonzero cap the plan allows (and one nonzero past it: the VALU fallback), and
p - 1 everywhere in all five fields.  Every comparison is of the whole of y: what a launch must
not write holds a sentinel that is no field element.  Every Ft127 case runs on the matrix cores
(used_mfma says so) and again on the VALU kernel.  The Reed-Solomon step under the last level
(lcpc_selftest_reed_solomon) gets the same extremes, and one encode through the public API ties
both kernels of a real plan to the oracle on p - 1 messages."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import field_ref as FR
import mfma_adv as ADV

pytestmark = pytest.mark.gpu

FT127 = 1
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)  # a top limb above every field's p
SPMM_SPLIT_BELOW = 2048  # csrc/sdig.hip: fewer outputs take the four-waves-per-output kernel
MFMA_MAX_NNZ = 512       # 4 SPMM_MAX_GROUPS: one nonzero more sends the whole matrix to the VALU kernel
ONE_WAVE_OUTPUTS = 2051  # >= SPMM_SPLIT_BELOW, and a last block of three live waves


def mfma_tiling(R):
    """mfma_tiling of csrc/sdig.hip, restated: (tiles of 16 rows per wave, row chunks)."""
    chunks = (R + 127) // 128
    return (R + 16 * chunks - 1) // (16 * chunks), chunks


# R -> (tiles, chunks) as the issue's table has them; all with b0 = 0, nb = R
ALL_R = {1: (1, 1), 16: (1, 1), 17: (2, 1), 33: (3, 1), 49: (4, 1), 65: (5, 1), 81: (6, 1), 97: (7, 1),
         113: (8, 1), 128: (8, 1), 129: (5, 2), 256: (8, 2), 257: (6, 3)}


def test_r_list_reaches_every_tile_and_chunk_count():
    got = {R: mfma_tiling(R) for R in ALL_R}
    assert got == ALL_R
    tiles, chunks = {t for t, _ in got.values()}, {c for _, c in got.values()}
    print(f"tile counts reached: {sorted(tiles)}, chunk counts reached: {sorted(chunks)}")
    assert tiles == set(range(1, 9)) and len(chunks) >= 3
    assert 129 % 128 and mfma_tiling(129)[0] * 16 * 2 > 129  # a partial last chunk


class Csr:
    """A CSR matrix by output: counts[j] nonzeros of output j, idx and val (integers) per nonzero."""

    def __init__(self, fr, m_cols, counts, idx, val):
        assert len(idx) == len(val) == sum(counts) and all(i < m_cols for i in idx)
        self.fr, self.m_cols, self.counts, self.idx, self.val = fr, m_cols, list(counts), list(idx), list(val)
        self.ptr = [0]
        for c in counts:
            self.ptr.append(self.ptr[-1] + c)
        self.m_rows = len(counts)
        self.val_arr = fr.to_array(val) if val else np.zeros((0, fr.nl), np.uint64)

    def reference(self, x):
        """x[i][b] integers -> y[j][b] integers."""
        fr, R = self.fr, len(x[0])
        out = []
        for j in range(self.m_rows):
            ks = range(self.ptr[j], self.ptr[j + 1])
            vs, cols = [self.val[k] for k in ks], [x[self.idx[k]] for k in ks]
            out.append([sum(v * c[b] for v, c in zip(vs, cols)) * fr.Rinv % fr.p for b in range(R)])
        return out


def _arr(fr, grid):
    """[n][R] integers -> (n, R, limbs) words."""
    R = len(grid[0])
    return fr.to_array([v for row in grid for v in row]).reshape(len(grid), R, fr.nl)


def _run_and_compare(gpu, m, x_arr, want_arr, b0=0, nb=None, expect_mfma=None):
    """Both paths for Ft127 (path 0 on the matrix cores unless expect_mfma says otherwise), path 0
    for the other fields; all of y against want inside [b0, b0 + nb) and the sentinel outside."""
    fr, R = m.fr, x_arr.shape[1]
    nb = R - b0 if nb is None else nb
    exp = np.full((m.m_rows, R, fr.nl), SENTINEL, np.uint64)
    exp[:, b0:b0 + nb] = want_arr[:, b0:b0 + nb]
    if expect_mfma is None:
        expect_mfma = 1 if fr.fid == FT127 and nb and m.m_rows else 0
    for path in ((0, 1) if fr.fid == FT127 else (0,)):
        y = np.full((m.m_rows, R, fr.nl), SENTINEL, np.uint64)
        _, used = gpu.selftest_spmm(fr.fid, m.ptr, m.idx, m.val_arr, x_arr, y, b0=b0, nb=nb, path=path)
        assert used == (expect_mfma if path == 0 else 0), f"path {path}: used_mfma = {used}"
        bad = np.argwhere((y != exp).any(axis=2))
        assert not len(bad), f"path {path} (used_mfma {used}): {len(bad)} elements differ, first (output, row) {bad[0]}"


# ---------------------------------------------------------------- the two matrix shapes
SPLIT_COUNTS = [0, 1, 3, 4, 5, 16, 17]  # groups of 4: 0, 1, 1, 1, 2, 4, 5 against the block's four waves
SPLIT_COLS = 11


@functools.lru_cache(maxsize=None)
def split_matrix():
    """7 outputs (the four-waves-per-output kernel).  The outputs with 16 and 17 nonzeros read 11
    inputs, so they repeat input indices."""
    fr = FR.field_ref(FT127)
    rng = random.Random(0x5D16)
    idx = [(3 * j + 5 * k) % SPLIT_COLS for j, c in enumerate(SPLIT_COUNTS) for k in range(c)]
    m = Csr(fr, SPLIT_COLS, SPLIT_COUNTS, idx, [rng.randrange(fr.p) for _ in idx])
    assert any(len(set(m.idx[m.ptr[j]:m.ptr[j + 1]])) < m.counts[j] for j in range(m.m_rows))
    return m


@functools.lru_cache(maxsize=None)
def one_wave_matrix():
    """2051 outputs (one wave per output), nonzero counts 0..5 in turn over 64 inputs."""
    fr = FR.field_ref(FT127)
    rng = random.Random(0x0E7A)
    counts = [j % 6 for j in range(ONE_WAVE_OUTPUTS)]
    assert ONE_WAVE_OUTPUTS >= SPMM_SPLIT_BELOW and ONE_WAVE_OUTPUTS % 4 == 3
    n = sum(counts)
    return Csr(fr, 64, counts, [rng.randrange(64) for _ in range(n)], [rng.randrange(fr.p) for _ in range(n)])


MATRICES = {"split": split_matrix, "one_wave": one_wave_matrix}


@functools.lru_cache(maxsize=None)
def random_case(which, R):
    """(matrix, x words, expected y words) with random x: computed once, shared, not modified."""
    m = MATRICES[which]()
    rng = random.Random(1000 * R + len(which))
    x = [[rng.randrange(m.fr.p) for _ in range(R)] for _ in range(m.m_cols)]
    return m, _arr(m.fr, x), _arr(m.fr, m.reference(x))


@pytest.mark.parametrize("R", sorted(ALL_R))
@pytest.mark.parametrize("which", ["split", "one_wave"])
def test_spmm_every_instantiation(gpu, which, R):
    m, x_arr, want = random_case(which, R)
    assert (m.m_rows < SPMM_SPLIT_BELOW) == (which == "split") and max(m.counts) <= MFMA_MAX_NNZ
    _run_and_compare(gpu, m, x_arr, want)


@pytest.mark.parametrize("b0,nb", [(0, 200), (16, 130), (5, 17), (199, 1), (0, 0)])
@pytest.mark.parametrize("which", ["split", "one_wave"])
def test_spmm_row_sub_range(gpu, which, b0, nb):
    """Rows [b0, b0 + nb) of R = 200: a tile-aligned and two unaligned starts, a range of two
    chunks, the last row alone, and the empty range (no launch: used_mfma = 0)."""
    m, x_arr, want = random_case(which, 200)
    _run_and_compare(gpu, m, x_arr, want, b0=b0, nb=nb)


# ---------------------------------------------------------------- the accumulator bound
# One output has n nonzeros, each of value T, and every input it reads holds the x that
# mfma_adv builds for (T, u, s): Y_v of that output is n times the pair's sums.
ADV_R = 17  # a full tile and a one-row tile


@functools.lru_cache(maxsize=None)
def adversarial_pair(u, s):
    """(T, x, the pair's 16 sums) for the target: the best-scoring T whose model stays inside the
    kernel's stated domain at 512 nonzeros, |Y_v| < 2^27 for every v."""
    fr = FR.field_ref(FT127)
    for T in ADV.adversarial_tensor_words(fr, ADV.ADV_KEPT):
        h = ADV.residue_digits(fr, T)
        x = ADV.adversarial_coefficient(fr, h, u, s)
        sums = ADV.pair_sums(h, x)
        if MFMA_MAX_NNZ * max(abs(v) for v in sums) < 1 << 27:
            return T, x, sums
    raise AssertionError("no candidate T keeps the model below 2^27")


def _model_check(u, s, n):
    T, x, sums = adversarial_pair(u, s)
    top = n * max(abs(v) for v in sums)
    print(f"sdig adversarial (u, s) = ({u}, {s}), {n} nonzeros: largest |Y| = {top} = 2^{np.log2(top):.3f}, "
          f"{top / 2**27:.4f} of 2^27 (target Y_u = {n * sums[u]})")
    assert sums[u] * s >= ADV.ADV_PER_ROW
    if n == MFMA_MAX_NNZ:
        assert 1 << 26 <= top < 1 << 27
    return T, x


def _adversarial_case(counts, u, s, m_cols=3):
    fr = FR.field_ref(FT127)
    T, x = _model_check(u, s, MFMA_MAX_NNZ)
    n = sum(counts)
    m = Csr(fr, m_cols, counts, [k % m_cols for k in range(n)], [T] * n)
    xs = [[x] * ADV_R for _ in range(m_cols)]  # input 0 too: the pads of a last group read it
    want = m.reference(xs)
    assert want[0][0] == counts[0] * T * x * fr.Rinv % fr.p  # every product is T x
    return m, _arr(fr, xs), _arr(fr, want)


@pytest.mark.parametrize("u,s", ADV.ADV_TARGETS)
def test_spmm_accumulator_bound_split(gpu, u, s):
    """512 nonzeros (the cap), and 509, 510, 511: the zero-valued pads of the last group add
    nothing.  7 outputs: four waves share each output's 128 groups."""
    m, x_arr, want = _adversarial_case([512, 509, 0, 510, 511, 5, 512], u, s)
    _run_and_compare(gpu, m, x_arr, want)


@pytest.mark.parametrize("u,s", ADV.ADV_TARGETS)
def test_spmm_accumulator_bound_one_wave(gpu, u, s):
    """The same at 2051 outputs: one wave walks all 128 groups of an output.  The first, a middle
    and the last output (the third wave of the last block) hold 512 nonzeros, one 511, the rest
    0..5 in turn."""
    counts = [j % 6 for j in range(ONE_WAVE_OUTPUTS)]
    counts[0] = counts[1026] = counts[ONE_WAVE_OUTPUTS - 1] = 512
    counts[7] = 511
    m, x_arr, want = _adversarial_case(counts, u, s)
    _run_and_compare(gpu, m, x_arr, want)


def test_spmm_513_nonzeros_fall_back_to_valu(gpu):
    """One output past the cap: the plan keeps the VALU kernel for the whole matrix, so path 0
    reports used_mfma = 0, and the result is still the reference's."""
    u, s = ADV.ADV_TARGETS[0]
    m, x_arr, want = _adversarial_case([3, 513, 0, 4, 512], u, s)
    _run_and_compare(gpu, m, x_arr, want, expect_mfma=0)


# ---------------------------------------------------------------- extremes, all fields
EXT_R, EXT_COLS = 5, 6


@pytest.mark.parametrize("pattern", ["max", "alternating"])
@pytest.mark.parametrize("fid", FR.FIDS)
def test_spmm_extremes(gpu, fid, pattern):
    """Nonzero counts 0..9 per output: every remainder of k_spmm's K-group loop for K = 1..4
    (K = min(fe_dot_kmax, 4)).  "max": every value and every x is p - 1, so fe_dot<K> sums
    K (p - 1)^2; for Ft127 one more output holds 512 nonzeros of p - 1.  "alternating": 0 and
    p - 1 in turn along inputs and rows, and along the nonzeros with another period."""
    fr = FR.field_ref(fid)
    top = fr.p - 1
    counts = list(range(10)) + ([MFMA_MAX_NNZ] if fid == FT127 and pattern == "max" else [])
    idx = [(j + k) % EXT_COLS for j, c in enumerate(counts) for k in range(c)]
    if pattern == "max":
        val = [top] * len(idx)
        x = [[top] * EXT_R for _ in range(EXT_COLS)]
    else:
        val = [0 if k % 3 == 2 else top for k in range(len(idx))]
        x = [[top if (i + b) % 2 else 0 for b in range(EXT_R)] for i in range(EXT_COLS)]
    m = Csr(fr, EXT_COLS, counts, idx, val)
    _run_and_compare(gpu, m, _arr(fr, x), _arr(fr, m.reference(x)))


# ---------------------------------------------------------------- the Reed-Solomon step
# k_reed_solomon: out[k][b] = sum_j in[j][b] (k + 1)^j by Horner.  Its inputs in an encode are
# the last precode's outputs, so the public API cannot hand it p - 1 either.  (lcpc_selftest_reed_solomon)
RS_M, RS_OUT, RS_R = 23, 301, 5  # more outputs x rows than one block of 256 threads, an odd count


@pytest.mark.parametrize("pattern", ["max", "alternating", "random", "empty"])
@pytest.mark.parametrize("fid", FR.FIDS)
def test_reed_solomon_step(gpu, fid, pattern):
    fr = FR.field_ref(fid)
    top, rng = fr.p - 1, random.Random(0x85 + fid)
    m = 0 if pattern == "empty" else RS_M  # no input: every output is zero
    if pattern == "max":
        inp = [[top] * RS_R for _ in range(m)]
    elif pattern == "alternating":
        inp = [[top if (j + b) % 2 else 0 for b in range(RS_R)] for j in range(m)]
    else:
        inp = [[rng.randrange(fr.p) for _ in range(RS_R)] for _ in range(m)]
    want = [[sum(inp[j][b] * pow(k + 1, j, fr.p) for j in range(m)) % fr.p for b in range(RS_R)]
            for k in range(RS_OUT)]
    inp_arr = _arr(fr, inp) if m else np.zeros((0, RS_R, fr.nl), np.uint64)
    want_arr = _arr(fr, want)
    for b0, nb in [(0, RS_R), (1, 3), (RS_R - 1, 1), (2, 0)]:
        exp = np.full((RS_OUT, RS_R, fr.nl), SENTINEL, np.uint64)
        exp[:, b0:b0 + nb] = want_arr[:, b0:b0 + nb]
        out = np.full((RS_OUT, RS_R, fr.nl), SENTINEL, np.uint64)
        gpu.selftest_reed_solomon(fid, inp_arr, out, b0=b0, nb=nb)
        bad = np.argwhere((out != exp).any(axis=2))
        assert not len(bad), f"rows [{b0}, {b0 + nb}): {len(bad)} elements differ, first (output, row) {bad[0]}"


# ---------------------------------------------------------------- through the public API once
API_NP, API_SEED, API_CODE = 16384, 0, 3


def _oracle_level_outputs(oracle, enc):
    L = oracle.lib()
    dims = []
    for lvl in range(L.of_sdig_levels(enc.ptr)):
        for which in (0, 1):
            r, c = C.c_size_t(), C.c_size_t()
            L.of_sdig_matrix(enc.ptr, lvl, which, C.byref(r), C.byref(c), None, None, None)
            dims.append((["pre", "post"][which], lvl, r.value))
    return dims


@pytest.mark.parametrize("R", [1, 130])
def test_sdig_encode_rows_extremes_both_kernels(gpu, oracle, R):
    """Ft127, SdigCode3, seed 0, n_per_row = 16384: the outputs per level (sdig_level_dims; the
    oracle's matrices have the same shapes) are
        pre  2917, 520, 93, 17        post 4100, 729, 129, 23        (n_cols = 24921)
    so pre0 and post0 (>= 2048) take the one-wave kernel and the six deeper levels the split
    kernel, in one encode.  Messages: p - 1 everywhere, and 0 / p - 1 in a checkerboard over (row, element); R = 130 is
    two row chunks of five tiles."""
    fr = FR.field_ref(FT127)
    o = oracle.Encoding.sdig(FT127, API_NP, seed=API_SEED, code_id=API_CODE)
    outs = [n for _, _, n in _oracle_level_outputs(oracle, o)]
    print("outputs per level:", _oracle_level_outputs(oracle, o))
    assert outs == [2917, 4100, 520, 729, 93, 129, 17, 23]  # (pre, post) per level
    assert any(n >= SPMM_SPLIT_BELOW for n in outs) and any(0 < n < SPMM_SPLIT_BELOW for n in outs)
    g = gpu.SdigEncoding.new_from_dims(FT127, API_NP, o.n_cols, API_SEED, API_CODE)
    top = fr.to_array([fr.p - 1])[0]
    for pattern in ("max", "checkerboard"):
        rows = np.zeros((R, o.n_cols, fr.nl), np.uint64)
        if pattern == "max":
            rows[:, :API_NP] = top
        else:
            on = (np.arange(R)[:, None] + np.arange(API_NP)[None, :]) % 2 == 1
            rows[:, :API_NP][on] = top
        want = {}
        for r in range(min(R, 2)):  # at most two distinct rows
            want[r] = o.encode(rows[r].reshape(-1).copy())
        got = g.encode_rows(rows.copy())
        for r in range(R):
            assert np.array_equal(got[r].reshape(-1), want[r % 2 if pattern == "checkerboard" else 0]), (pattern, r)
