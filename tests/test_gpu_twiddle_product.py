"""GPU: the word-expanded twiddle product of csrc/field.hpp (fe_mul_tw) and the table kernel that
feeds it (fe_tw_expand), Ft127, against Python integers.

For a constant w the table keeps W_i = w 2^(32 (i + 2)) mod p, i < 4, each fully reduced; for
x = sum_i x_i 2^(32 i) the product forms T = sum_i x_i W_i and applies two Montgomery word-steps,
y = (T + m_0 p + m_1 p 2^32) / 2^64.  That integer is unique, so every product below is compared
with it word for word -- which implies the two properties the NTT passes rely on and which are
asserted on their own as well: y < 2p and y = x w (mod p), the class fe_mul_lazy(x, w R) returns.

Operands: x over the edges of [0, 2p) (0, 1, p - 1, p, p + 1, 2p - 1, 2^127, one limb of all ones,
2p - 1 with one limb cleared) crossed with w in {0, 1, 2, p - 1, p - 2, omega, omega^-1} and with
constants solved for so that one W_i has its top word equal to p_3 (the bound tw_free_mask takes
for column 3) or its low words all ones; 2^16 random pairs with x uniform in [0, 2p); and word
groups that belong to no single w (every W_i = p - 1, ...), which the primitive's contract -- any
W_i < p -- covers.  x = 0xffffffff 2^96 is >= 2p, outside the domain, and is left out.
"""
import random

import numpy as np
import pytest

import field_ref as FR

pytestmark = pytest.mark.gpu

FID, N = 1, 4
M32 = 0xFFFFFFFF


def _fr():
    return FR.field_ref(FID)


def _expand(fr, w):
    return [w * pow(2, 32 * (i + 2), fr.p) % fr.p for i in range(N)]


def _two_steps(fr, x, W):
    T = sum(((x >> (32 * i)) & M32) * W[i] for i in range(N))
    for _ in range(2):
        T = (T + ((-T) & M32) * fr.p) >> 32
    return T


def _omega(oracle, fr, log_n=16):
    w = np.zeros(fr.nl, np.uint64)
    oracle.lib().of_ntt_omega(FID, log_n, oracle.p64(w))
    return fr.from_array(w)[0] * fr.Rinv % fr.p  # canonical value of the 2^16-point root


def _named_ws(oracle, fr):
    om = _omega(oracle, fr)
    return [0, 1, 2, fr.p - 1, fr.p - 2, om, pow(om, -1, fr.p)]


def _stress_ws(fr):
    """w with a chosen W_i: solve w = V 2^(-32 (i + 2)) for V with top word p_3 / low words all ones."""
    p, P = fr.p, fr.P
    rng = random.Random(0x7411)
    vals = []
    for i in range(N):
        inv = pow(2, -32 * (i + 2), p)
        top_p3 = [(P[3] << 96) | rng.randrange(P[2] << 64),            # top word p_3, the rest random (< p)
                  (P[3] << 96) | ((P[2] - 1) << 64) | ((1 << 64) - 1),  # ... and two low words of all ones
                  p - 1]
        low_ones = [(rng.randrange(P[3]) << 96) | ((1 << 96) - 1),      # three low words of all ones
                    ((P[3] - 1) << 96) | ((1 << 96) - 1)]
        for V in top_p3:
            assert V < p and V >> 96 == P[3]
        for V in low_ones:
            assert V < p and V & ((1 << 96) - 1) == (1 << 96) - 1
        vals += [V * inv % p for V in top_p3 + low_ones]
    for w in vals:  # the search's own check: some W_i of every w has the property
        W = _expand(fr, w)
        assert any(v >> 96 == P[3] for v in W) or any(v & ((1 << 96) - 1) == (1 << 96) - 1 for v in W)
    return vals


def _edge_xs(fr):
    p = fr.p
    xs = [0, 1, p - 1, p, p + 1, 2 * p - 1, 1 << 127]
    xs += [M32 << (32 * i) for i in range(N - 1)]  # (limb 3 of all ones is >= 2p: outside the domain)
    xs += [(2 * p - 1) & ~(M32 << (32 * i)) for i in range(N)]
    assert all(x < 2 * p for x in xs)
    return xs


def test_table_expansion_matches_integers(gpu, oracle):
    fr = _fr()
    rng = random.Random(0x7410)
    ws = _named_ws(oracle, fr) + _stress_ws(fr) + [rng.randrange(fr.p) for _ in range(4096)]
    mont = [w * fr.R % fr.p for w in ws]
    got = gpu.selftest_twiddle_words(FID, fr.to_array(mont))
    assert got.shape == (len(ws), N, fr.nl)
    got = fr.from_array(got.reshape(-1, fr.nl))
    want = [v for w in ws for v in _expand(fr, w)]
    assert max(got) < fr.p, "a word group is not canonical"
    assert got[2::N] == mont, "group 2 is not the Montgomery twiddle"
    bad = [k for k, (g, v) in enumerate(zip(got, want)) if g != v]
    assert not bad, f"{len(bad)} groups differ; first: w = {hex(ws[bad[0] // N])}, i = {bad[0] % N}, " \
                    f"got {hex(got[bad[0]])}, want {hex(want[bad[0]])}"


def _check_products(gpu, fr, xs, Ws, ws=None):
    """xs[k] times the word groups Ws[k] (of the constant ws[k], when there is one)."""
    b = fr.to_array([v for W in Ws for v in W])
    got = fr.from_array(gpu.selftest_field_op(FID, "mul_tw", fr.to_array(xs), b))
    for k, (x, W, y) in enumerate(zip(xs, Ws, got)):
        ctx = f"x = {hex(x)}, W = {[hex(v) for v in W]}, got {hex(y)}"
        assert y < 2 * fr.p, "raw output >= 2p: " + ctx
        if ws is not None:
            assert y % fr.p == x * ws[k] % fr.p, f"not congruent to x w, w = {hex(ws[k])}: " + ctx
        assert y == _two_steps(fr, x, W), f"want {hex(_two_steps(fr, x, W))}: " + ctx


def test_product_on_the_edges_of_the_domain(gpu, oracle):
    fr = _fr()
    consts = _named_ws(oracle, fr) + _stress_ws(fr)
    pairs = [(x, w) for x in _edge_xs(fr) for w in consts]
    xs, ws = [x for x, _ in pairs], [w for _, w in pairs]
    _check_products(gpu, fr, xs, [_expand(fr, w) for w in ws], ws)


def test_product_is_congruent_to_the_lazy_montgomery_product(gpu, oracle):
    """The same class as today's twiddle product: fe_mul_lazy(x, w R), on the edge operands."""
    fr = _fr()
    pairs = [(x, w) for x in _edge_xs(fr) for w in _named_ws(oracle, fr)]
    xs, ws = [x for x, _ in pairs], [w for _, w in pairs]
    lazy = fr.from_array(gpu.selftest_field_op(FID, "mul_lazy", fr.to_array(xs),
                                               fr.to_array([w * fr.R % fr.p for w in ws])))
    b = fr.to_array([v for w in ws for v in _expand(fr, w)])
    new = fr.from_array(gpu.selftest_field_op(FID, "mul_tw", fr.to_array(xs), b))
    assert [y % fr.p for y in new] == [y % fr.p for y in lazy]


def test_product_on_random_pairs(gpu):
    fr = _fr()
    rng = random.Random(0x7412)
    n = 1 << 16
    xs = [rng.randrange(2 * fr.p) for _ in range(n)]
    ws = [rng.randrange(fr.p) for _ in range(n)]
    _check_products(gpu, fr, xs, [_expand(fr, w) for w in ws], ws)


def test_product_on_word_groups_of_no_single_constant(gpu):
    """Every W_i at its own extreme at once (what the free mask's bounds are stated for): all p - 1,
    all top word p_3 with ones below, all low words of ones, and random mixtures."""
    fr = _fr()
    p, P = fr.p, fr.P
    rng = random.Random(0x7413)
    ext = [p - 1, (P[3] << 96) | ((P[2] - 1) << 64) | ((1 << 64) - 1), ((P[3] - 1) << 96) | ((1 << 96) - 1), 0, 1]
    groups = [[v] * N for v in ext] + [[rng.choice(ext + [rng.randrange(p)]) for _ in range(N)] for _ in range(2048)]
    pairs = [(x, W) for x in _edge_xs(fr) for W in groups[:len(ext)]]
    pairs += [(rng.choice(_edge_xs(fr) + [rng.randrange(2 * p)]), W) for W in groups[len(ext):]]
    _check_products(gpu, fr, [x for x, _ in pairs], [W for _, W in pairs])
