"""GPU: every primitive of csrc/field.hpp, and the Ft127 digit recombination of
csrc/collapse_mfma.hpp, one call per thread (lcpc_selftest_field_op / lcpc_selftest_recombine)
against Python integers (tests/field_ref.py), word for word, over operands chosen for the bounds
the code was proven under: p - 1, 2p - 1, limbs of all ones in both operands of one product,
quotient words of all ones, K (p - 1)^2 in fe_dot<K> for every K up to fe_dot_kmax, digit
accumulators at +-(2^27 - 1).  tests/test_field_ref.py checks the reference and the pool on the
CPU first.

A mismatch is a bug in field.hpp or collapse_mfma.hpp (or a stated bound that is wrong): the
failure message shows the first differing operands in hex.
"""
import numpy as np
import pytest

import field_ref as FR

pytestmark = pytest.mark.gpu

CASES = [(fid, name) for fid in FR.FIDS for name in FR.case_names(FR.field_ref(fid))]


def _first_difference(fr, name, k, a, b, got, want):
    na = 2 if name == "mul_sub_lazy" else k  # operands of a / of b per output
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    i = bad[0]
    xs = [hex(v) for v in a[i * na:(i + 1) * na]]
    ys = [hex(v) for v in b[i * k:(i + 1) * k]] if b is not None else None
    return f"{name} fid {fr.fid}: {len(bad)} of {len(want)} differ; first at {i}: a = {xs}, b = {ys}, " \
           f"got {hex(got[i])}, want {hex(want[i])}"


@pytest.mark.parametrize("fid,name", CASES, ids=[f"f{f}-{n}" for f, n in CASES])
def test_field_op_matches_integers(gpu, fid, name):
    fr = FR.field_ref(fid)
    op, k = FR.case_op(name)
    a, b = FR.operands(fr, name)
    want = fr.expected(op, a, b, k)
    if name == "mul_lazy":
        assert max(want) < 2 * fr.p
    got_arr = gpu.selftest_field_op(fid, op, fr.to_array(a), None if b is None else fr.to_array(b), k=k)
    want_arr = fr.to_array(want)
    if not np.array_equal(got_arr, want_arr):
        msg = _first_difference(fr, name, k, a, b, fr.from_array(got_arr), want)
        print(msg)
        pytest.fail(msg)


def test_fe_dot_kmax_is_the_cap(gpu):
    for fid in FR.FIDS:
        assert gpu.selftest_fe_dot_kmax(fid) == FR.field_ref(fid).dot_kmax
    assert gpu.selftest_fe_dot_kmax(gpu.FT253_192) == 8


def test_balanced_digits_properties(gpu):
    """Beyond equality with the reference's digits: 16 digits in [-128, 128) that sum to x, the
    top one never negative (what collapse_mfma.hpp's bound on the accumulators assumes)."""
    fr = FR.field_ref(1)
    xs = FR.pool(fr, "p")
    d = gpu.selftest_field_op(1, "balanced_digits", fr.to_array(xs)).view(np.int8).reshape(-1, 16)
    assert (d[:, 15] >= 0).all()
    for x, row in zip(xs, d):
        assert sum(int(v) << (8 * a) for a, v in enumerate(row)) == x


# ---------------------------------------------------------------- recombine_redc at its bound
BOUND = (1 << 27) - 1  # |Y_u| < 2^27: 512 rows x 16 digits x 2^14 per split


def _recombine_rows():
    fr = FR.field_ref(1)
    rows, names = [], []

    def add(name, row):
        names.append(name)
        rows.append([int(v) for v in row])

    add("all +bound", [BOUND] * 16)
    add("all -bound", [-BOUND] * 16)
    for u in (15, 0):
        for s in (1, -1):
            add(f"only Y{u} = {s * BOUND}", [s * BOUND if v == u else 0 for v in range(16)])
    add("alternating +-", [BOUND if u % 2 == 0 else -BOUND for u in range(16)])
    add("alternating -+", [-BOUND if u % 2 == 0 else BOUND for u in range(16)])
    add("all zero", [0] * 16)
    dp = FR.balanced_digits(fr.p)
    add("sum = +p", dp)
    add("sum = -p", [-v for v in dp])
    add("sum = +1", [1] + [0] * 15)
    add("sum = -1", [-1] + [0] * 15)
    # the same sums in spread-out form: +-p and +-1 with every accumulator at the bound's scale
    spread = [BOUND] * 15
    low = sum(v << (8 * u) for u, v in enumerate(spread))
    for target, label in ((fr.p, "+p"), (-fr.p, "-p"), (1, "+1"), (-1, "-1")):
        # Y_15 2^120 + low = target mod p, |Y_15| < 2^27: solve for Y_15 mod p and keep small ones
        y15 = (target - low) * pow(1 << 120, -1, fr.p) % fr.p
        if y15 > fr.p // 2:
            y15 -= fr.p
        if abs(y15) <= BOUND:
            add(f"sum = {label} mod p, spread", spread + [y15])
    rng = np.random.default_rng(0x5EC0)
    named = len(rows)
    big = rng.integers(-BOUND, BOUND + 1, size=(4096, 16), dtype=np.int64)
    small = rng.integers(-(1 << 12) + 1, 1 << 12, size=(4096, 16), dtype=np.int64)
    y = np.concatenate([np.array(rows, dtype=np.int64), big, small]).astype(np.int32)
    names += ["random within the bound"] * 4096 + ["random below 2^12"] * 4096
    assert named >= 13 and np.abs(y).max() == BOUND
    return fr, y, names


def test_recombine_redc_at_the_bound(gpu):
    fr, y, names = _recombine_rows()
    want = FR.recombine_expected(fr, y.tolist())
    assert all(0 <= w < fr.p for w in want)
    got = fr.from_array(gpu.selftest_recombine(y))
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    if bad:
        i = bad[0]
        msg = f"recombine_redc: {len(bad)} of {len(want)} differ; first: {names[i]}, Y = " \
              f"{[hex(int(v)) for v in y[i]]}, got {hex(got[i])}, want {hex(want[i])}"
        print(msg)
        pytest.fail(msg)
