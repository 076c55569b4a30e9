"""GPU: the row combinations (collapse_columns, lcpc-2d/src/lib.rs:1126-1154) for 1 to 4
tensors at once, through a row shard holding every row (lcpc_shard_collapse and its
device-resident form), against the oracle tensor by tensor.  For Ft127 with up to 3 tensors
this is the int8 matrix-core kernel (collapse_mfma.hpp); 4 tensors and the other fields take
the VALU kernel.  Shapes cover ragged rows and columns (not multiples of the 4-row MFMA step or
the 64-column wave tile), one row, and more rows than one 512-row split.  Random data keeps the
matrix-core accumulators near 2^17; the second half builds coefficients from the tensor's own
digits so that they grow as fast as any input can make them, and runs the plain extremes
(p - 1 everywhere, 0 alternating with p - 1), against Python integers and the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(37, 100), (1, 64), (4, 1000), (600, 70), (512, 4096)]


@pytest.mark.parametrize("fid", [1, 0, 2, 3])
@pytest.mark.parametrize("n_rows,n_per_row", SHAPES)
@pytest.mark.parametrize("n_t", [1, 2, 3, 4])
def test_collapse_tensors_match_oracle(gpu, oracle, fid, n_rows, n_per_row, n_t):
    from lcpc_proof_of_storage_amd.shard import GpuBackend
    if fid in (2, 3) and n_rows * n_per_row > 100000:
        pytest.skip("Ft191 / Ft255: the small shapes suffice")
    nl = oracle.limbs(fid)
    n_cols = 1 << (n_per_row.bit_length())
    enc = gpu.LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
    be = GpuBackend(enc)
    rng = oracle.ChaCha(seed_u64=n_rows * 1000 + n_per_row + n_t)
    coeffs = rng.field_random(fid, n_rows * n_per_row).reshape(n_rows, n_per_row * nl)
    tens = rng.field_random(fid, n_t * n_rows).reshape(n_t, n_rows, nl)
    sh = be.shard_new(coeffs, 0, n_rows)
    try:
        got = be.collapse(sh, tens)
        for t in range(n_t):
            want = oracle.collapse(fid, coeffs, tens[t], n_rows, n_per_row)
            assert np.array_equal(got[t].reshape(-1), want), f"tensor {t}"
    finally:
        be.shard_free(sh)


@pytest.mark.parametrize("n_t", [1, 2, 3])
def test_collapse_device_form_matches_host_form(gpu, oracle, n_t):
    import torch
    from lcpc_proof_of_storage_amd.shard import GpuBackend
    fid, n_rows, n_per_row = 1, 300, 2048
    nl = oracle.limbs(fid)
    enc = gpu.LigeroEncoding.new_from_dims(fid, n_per_row, 4096)
    be = GpuBackend(enc)
    rng = oracle.ChaCha(seed_u64=77 + n_t)
    coeffs = rng.field_random(fid, n_rows * n_per_row).reshape(n_rows, n_per_row * nl)
    tens = rng.field_random(fid, n_t * n_rows).reshape(n_t, n_rows, nl)
    sh = be.shard_new(coeffs, 0, n_rows)
    try:
        host = be.collapse(sh, tens)
        dt = torch.from_numpy(np.ascontiguousarray(tens).view(np.int64)).to("cuda:0")
        dev = be.collapse_dev(sh, dt).cpu().numpy().view(np.uint64)
        assert np.array_equal(dev, host)
    finally:
        be.shard_free(sh)


# ---------------------------------------------------------------- adversarial row combinations
# Random digits have random signs, so at the shapes above the matrix-core accumulators stay near
# 2^17 of the 2^27 recombine_redc allows.  Here every row of a tensor holds one Montgomery word T
# and every row of a column one coefficient x built from the digits of T's residues
# h[a][u] = bal(T 2^(8a) mod p): for a digit position u and a sign s, d_a = 127 where h[a][u] has
# sign s and -128 elsewhere, so that every product h[a][u] d_a of the column has the same sign and
# Y_u grows by about 2^17 per row, the most any coefficient can give.
ADV_SHAPES = [(64, 70), (600, 70), (37, 100)]
# The search for T and the construction of x live in mfma_adv.py, shared with the sparse levels of
# sdig.hip (test_gpu_sdig_levels.py), which use the same digit scheme.
from mfma_adv import ADV_PER_ROW, ADV_TARGETS  # noqa: E402
from mfma_adv import adversarial_coefficient as _adversarial_coefficient  # noqa: E402
from mfma_adv import adversarial_tensor_words as _adversarial_tensor_words  # noqa: E402
from mfma_adv import residue_digits as _residue_digits  # noqa: E402


def _mfma_rows_per_split(n_rows, n_per_row):
    """mfma_splits_for of csrc/collapse.hip, restated: the rows one accumulator sums."""
    blocks_x = (n_per_row + 255) // 256
    splits = min((512 + blocks_x - 1) // blocks_x, (n_rows + 15) // 16)
    splits = max(splits, (n_rows + 511) // 512, 1)
    return (n_rows + splits - 1) // splits


@pytest.mark.parametrize("n_rows,n_per_row", ADV_SHAPES)
@pytest.mark.parametrize("n_t", [1, 2, 3])
def test_collapse_mfma_adversarial_digits(gpu, oracle, n_rows, n_per_row, n_t):
    import field_ref as FR
    from lcpc_proof_of_storage_amd.shard import GpuBackend
    fid = 1
    fr = FR.field_ref(fid)
    Ts = _adversarial_tensor_words(fr, n_t)
    hs = [_residue_digits(fr, T) for T in Ts]
    # column c targets tensor c mod n_t and the (u, s) pairs in turn
    xs, per_row_max = [], 0
    for c in range(n_per_row):
        t = c % n_t
        u, s = ADV_TARGETS[(c // n_t) % len(ADV_TARGETS)]
        x = _adversarial_coefficient(fr, hs[t], u, s)
        xs.append(x)
        d = FR.balanced_digits(x)
        assert d[:15] == [127 if hs[t][a][u] * s > 0 else -128 for a in range(15)] and d[15] >= 0
        # the test's own integer model of the accumulators: per row of a split, Y_v of (tensor, column)
        y_target = sum(hs[t][a][u] * d[a] for a in range(16))
        assert y_target * s >= ADV_PER_ROW, (c, t, u, s, y_target)
        for tt in range(n_t):
            per_row_max = max(per_row_max, max(abs(sum(hs[tt][a][v] * d[a] for a in range(16))) for v in range(16)))
    rps = _mfma_rows_per_split(n_rows, n_per_row)
    print(f"collapse adversarial ({n_rows}, {n_per_row}), {n_t} tensors: {rps} rows per split, largest |Y| = "
          f"{rps * per_row_max} = 2^{np.log2(rps * per_row_max):.2f}, per 512 rows {512 * per_row_max / 2**27:.3f} of 2^27")
    assert rps * per_row_max < 1 << 27
    coeffs = np.tile(fr.to_array(xs).reshape(1, -1), (n_rows, 1))
    tens = np.stack([np.tile(fr.to_array([T]), (n_rows, 1)) for T in Ts])
    want = [[n_rows * T * x * fr.Rinv % fr.p for x in xs] for T in Ts]
    be = GpuBackend(gpu.LigeroEncoding.new_from_dims(fid, n_per_row, 1 << n_per_row.bit_length()))
    sh = be.shard_new(coeffs, 0, n_rows)
    try:
        got = be.collapse(sh, tens)
        for t in range(n_t):
            assert np.array_equal(oracle.collapse(fid, coeffs, tens[t], n_rows, n_per_row), fr.to_array(want[t]).reshape(-1))
            assert fr.from_array(got[t]) == want[t], f"tensor {t}"
    finally:
        be.shard_free(sh)


@pytest.mark.parametrize("fid,n_t", [(1, 1), (1, 2), (1, 3), (1, 4), (0, 1), (0, 4), (2, 1), (2, 4), (3, 1), (3, 4)])
@pytest.mark.parametrize("n_rows,n_per_row", ADV_SHAPES)
@pytest.mark.parametrize("pattern", ["max", "alternating"])
def test_collapse_extremes(gpu, oracle, fid, n_t, n_rows, n_per_row, pattern):
    """Every coefficient and tensor entry p - 1 (the VALU kernel's fe_dot<K> then sums K (p - 1)^2,
    the matrix-core kernel's digits are those of p - 1 in every row), and 0 alternating with p - 1
    along the rows and columns of the coefficients."""
    import field_ref as FR
    from lcpc_proof_of_storage_amd.shard import GpuBackend
    fr = FR.field_ref(fid)
    top = fr.p - 1
    if pattern == "max":
        grid = [[top] * n_per_row for _ in range(n_rows)]
    else:
        grid = [[top if (r + c) % 2 else 0 for c in range(n_per_row)] for r in range(n_rows)]
    coeffs = fr.to_array([v for row in grid for v in row]).reshape(n_rows, n_per_row * fr.nl)
    tens = np.tile(fr.to_array([top]), (n_t, n_rows, 1))
    count = [sum(1 for r in range(n_rows) if grid[r][c]) for c in range(n_per_row)]
    want = [k * top * top * fr.Rinv % fr.p for k in count]
    be = GpuBackend(gpu.LigeroEncoding.new_from_dims(fid, n_per_row, 1 << n_per_row.bit_length()))
    sh = be.shard_new(coeffs, 0, n_rows)
    try:
        got = be.collapse(sh, tens)
        assert np.array_equal(oracle.collapse(fid, coeffs, tens[0], n_rows, n_per_row), fr.to_array(want).reshape(-1))
        for t in range(n_t):
            assert fr.from_array(got[t]) == want, f"tensor {t}"
    finally:
        be.shard_free(sh)
