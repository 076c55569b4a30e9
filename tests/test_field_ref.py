"""CPU: the big-integer reference of tests/field_ref.py and its operand pool, before they are
held against a kernel (tests/test_gpu_field_ops.py):

* the reference's Montgomery product and conversions agree with the C oracle over the pool, and
  its closed-form reduction with its own word-serial one;
* redc(a b) < 2p over the lazy domain (a < 2p, b < p), the bound fe_mul_lazy's callers rely on;
* the pool is what field_ref says: every class non-empty and inside its domain, at least 10 000
  pairs per multiplicative op, the all-0xffffffff quotient pair present (or its best substitute
  recorded);
* the new self-test entries refuse bad arguments before they touch a device.
"""
import ctypes as C

import numpy as np
import pytest

import field_ref as FR

INVALID_ARG = 30


@pytest.fixture(scope="module", params=FR.FIDS)
def fr(request):
    return FR.field_ref(request.param)


def test_reference_matches_oracle(fr, oracle):
    fid = fr.fid
    assert oracle.modulus(fid) == fr.p and oracle.limbs(fid) == fr.nl
    a, b = FR.mul_pairs(fr, "p")
    got = fr.from_array(oracle.mul(fid, fr.to_array(a), fr.to_array(b)))
    assert got == fr.expected("mul", a, b)
    pp = FR.pool(fr, "p")
    assert fr.from_array(oracle.to_mont(fid, pp)) == fr.expected("to_mont", pp)
    assert oracle.from_mont(fid, fr.to_array(pp)) == fr.expected("from_mont", pp)


def test_closed_form_reduction_is_the_word_serial_one(fr):
    a, b = FR.mul_pairs(fr, "2p")
    for x, y in list(zip(a, b))[::7]:
        assert fr.redc(x * y) == fr.redc_words(x * y)[0]
    for x in FR.pool(fr, "R"):
        assert fr.redc(x) == fr.redc_words(x)[0] <= fr.p


def test_lazy_product_stays_below_2p(fr):
    a, b = FR.mul_pairs(fr, "2p")
    assert max(a) == 2 * fr.p - 1 and max(b) == fr.p - 1
    worst = max(fr.expected("mul_lazy", a, b))
    assert worst < 2 * fr.p, hex(worst)
    # the largest product of the domain itself
    assert fr.redc((2 * fr.p - 1) * (fr.p - 1)) < 2 * fr.p


def test_pool_is_what_it_says(fr):
    p, R = fr.p, fr.R
    for domain, bound in (("p", p), ("2p", 2 * p), ("R", R)):
        named, alpha, pl = FR.named_values(fr, domain), FR.alphabet_values(fr, domain), FR.pool(fr, domain)
        assert named and alpha and len(set(pl)) == len(pl)
        assert all(0 <= v < bound for v in pl)
        assert {0, 1, 2, p - 1, p - 2, p - (1 << 32), (p + 1) // 2, (p - 1) // 2, R % p, R * R % p} <= set(named)
        for k in range(1, fr.N):
            assert {1 << (32 * k), (1 << (32 * k)) - 1} <= set(named)
        # about half of the drawn limbs are all ones (bringing a value into range changes some);
        # Ft63 takes the alphabet's full cross product instead
        limbs = [(v >> (32 * i)) & FR.M32 for v in alpha for i in range(fr.N - 1)]
        if fr.N > 2:
            assert sum(w == FR.M32 for w in limbs) * 3 >= len(limbs)
        else:
            assert len(alpha) >= 100 and FR.M32 in limbs
    assert {p, p + 1, 2 * p - 1, 2 * p - 2} <= set(FR.pool(fr, "2p"))
    canon = set(FR.pool(fr, "R"))
    assert {p, p + 1, p - 1, R - 1} <= canon
    for i in range(fr.N):  # decided at limb i, from either side
        assert any(v < p and v >> (32 * (i + 1)) == p >> (32 * (i + 1)) and
                   (v >> (32 * i)) & FR.M32 == fr.P[i] - 1 for v in canon) or fr.P[i] == 0
        assert any(v > p and v >> (32 * (i + 1)) == p >> (32 * (i + 1)) and
                   (v >> (32 * i)) & FR.M32 == fr.P[i] + 1 for v in canon) or fr.P[i] == FR.M32
    for name in ("mul", "mul_a_below_2p", "mul_cios", "mul_lazy", "mul_sub_lazy"):
        assert len(FR.operands(fr, name)[1]) >= 10000, name


def test_quotient_word_targets(fr):
    q = FR.quotient_pairs(fr)
    assert q["inv"] and q["zero"] and q["ones"]
    assert all(a < fr.p and b < fr.p for a, b in q["inv"] + q["zero"] + q["ones"])
    assert any(a & FR.M32 == FR.M32 and b & FR.M32 == FR.M32 for a, b in q["inv"])
    for a, b in q["inv"]:
        assert (a * b) & FR.M32 == 1 and fr.redc_words(a * b)[1][0] == FR.M32
    for a, b in q["zero"]:
        assert (a * b) & FR.M32 == 0 and fr.redc_words(a * b)[1][0] == 0
    # a b = p mod R has every quotient word all ones; it exists for every field here (about
    # p / R of the odd a give a b < p), so the substitute is never needed
    assert q["ones_words"] == fr.N
    for a, b in q["ones"]:
        assert fr.redc_words(a * b)[1] == [FR.M32] * fr.N


def test_dot_tuples_hold_the_cap_deciding_tuple(fr):
    assert fr.dot_kmax * fr.p < fr.R
    assert fr.dot_kmax == {0: 3, 1: 2, 2: 3, 3: 2, 4: 8}[fr.fid]
    for k in range(1, fr.dot_kmax + 1):
        a, b = FR.dot_tuples(fr, k)
        assert len(a) == len(b) == (FR.DOT_TUPLES + 1) * k
        assert a[-k:] == b[-k:] == [fr.p - 1] * k
        # the sum of K products stays below p R: one reduction lands below 2p
        assert k * (fr.p - 1) ** 2 < fr.p * fr.R
        assert fr.redc(k * (fr.p - 1) ** 2) < 2 * fr.p


def test_balanced_digits_and_recombination_reference():
    fr = FR.field_ref(1)
    for x in FR.pool(fr, "p"):
        d = FR.balanced_digits(x)
        assert all(-128 <= v < 128 for v in d) and d[15] >= 0
        assert sum(v << (8 * a) for a, v in enumerate(d)) == x
        assert FR.recombine_expected(fr, [d]) == [x * fr.Rinv % fr.p]


# ---------------------------------------------------------------- argument checks (no device needed)
@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    return N.load()


def test_fe_dot_kmax_entry(native):
    for fid in FR.FIDS:
        assert native.lcpc_selftest_fe_dot_kmax(fid) == FR.field_ref(fid).dot_kmax
    assert native.lcpc_selftest_fe_dot_kmax(4) == 8
    assert native.lcpc_selftest_fe_dot_kmax(5) == 0 and native.lcpc_selftest_fe_dot_kmax(-1) == 0


def test_field_op_refuses_bad_arguments(native):
    from lcpc_proof_of_storage_amd import SELFTEST_OPS
    buf = np.zeros(64, np.uint64)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    call = native.lcpc_selftest_field_op
    n_ops = len(SELFTEST_OPS)
    assert sorted(SELFTEST_OPS.values()) == list(range(n_ops))
    assert call(5, SELFTEST_OPS["add"], 1, ptr, ptr, ptr, 1) == INVALID_ARG
    assert call(-1, SELFTEST_OPS["add"], 1, ptr, ptr, ptr, 1) == INVALID_ARG
    assert call(1, n_ops, 1, ptr, ptr, ptr, 1) == INVALID_ARG
    assert call(1, -1, 1, ptr, ptr, ptr, 1) == INVALID_ARG
    for fid in FR.FIDS:
        kmax = FR.field_ref(fid).dot_kmax
        for k in (0, -1, kmax + 1):
            assert call(fid, SELFTEST_OPS["dot"], k, ptr, ptr, ptr, 1) == INVALID_ARG, (fid, k)
        if fid != 1:
            assert call(fid, SELFTEST_OPS["balanced_digits"], 1, ptr, None, ptr, 1) == INVALID_ARG
    assert call(1, SELFTEST_OPS["mul"], 1, None, ptr, ptr, 1) == INVALID_ARG
    assert call(1, SELFTEST_OPS["mul"], 1, ptr, None, ptr, 1) == INVALID_ARG
    assert call(1, SELFTEST_OPS["mul"], 1, ptr, ptr, None, 1) == INVALID_ARG
    assert call(1, SELFTEST_OPS["sqr"], 1, None, None, ptr, 1) == INVALID_ARG
    assert buf.sum() == 0


def test_recombine_refuses_null_pointers(native):
    y = np.zeros(16, np.int32)
    out = np.zeros(2, np.uint64)
    py, po = y.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(C.c_uint64))
    assert native.lcpc_selftest_recombine(None, po, 1) == INVALID_ARG
    assert native.lcpc_selftest_recombine(py, None, 1) == INVALID_ARG
