"""Adversarial operands for the Ft127 int8 matrix-core kernels (csrc/collapse_mfma.hpp's digit
scheme: the row combination of collapse.hip and the sparse levels of sdig.hip).  TEST
INFRASTRUCTURE ONLY, shared by test_gpu_collapse.py and test_gpu_sdig_levels.py.

Random digits have random signs, so on random data the digit-position accumulators stay near 2^17
of the 2^27 recombine_redc allows.  Here one operand is a Montgomery word T, the other a value x
built from the digits of T's residues h[a][u] = bal(T 2^(8a) mod p): for a digit position u and a
sign s, d_a = 127 where h[a][u] has sign s and -128 elsewhere, so that every product h[a][u] d_a
has the same sign and Y_u grows by about 2^17 per (T, x) pair, the most any x can give."""
import random

import field_ref as FR

ADV_TARGETS = [(u, s) for u in (0, 7, 14, 15) for s in (1, -1)]
ADV_PER_ROW = (1 << 26) // 512  # the floor the tests assert: half of the 2^27 bound per 512 pairs
ADV_CANDIDATES = 20000
ADV_KEPT = 16  # candidates kept from the search, best first


def residue_digits(fr, T):
    return [FR.balanced_digits((T << (8 * a)) % fr.p) for a in range(16)]  # h[a][u]


_ADV_WORDS = {}


def adversarial_tensor_words(fr, n_t):
    """The n_t best T of a fixed-seed search (done once): the candidates whose smallest
    sum_a |h[a][u]| over the targeted digit positions is largest."""
    if not _ADV_WORDS:
        _ADV_WORDS[0] = search_tensor_words(fr, ADV_KEPT)
    return _ADV_WORDS[0][:n_t]


def search_tensor_words(fr, n_t):
    rng = random.Random(0xADC0)
    cands = [rng.randrange(fr.p) for _ in range(ADV_CANDIDATES)]
    off = int.from_bytes(b"\x80" * 16, "little")
    us = sorted({u for u, _ in ADV_TARGETS})

    def score(T):
        tot = [0] * 16
        for a in range(16):
            for u, byte in enumerate((((T << (8 * a)) % fr.p) + off).to_bytes(16, "little")):
                tot[u] += abs(byte - 128)
        return min(tot[u] for u in us)
    return sorted(cands, key=score, reverse=True)[:n_t]


def adversarial_coefficient(fr, h, u, s):
    """x in [0, p) whose digits d_a (a < 15) are 127 where h[a][u] has sign s, else -128."""
    d = [127 if h[a][u] * s > 0 else -128 for a in range(15)]
    low = sum(v << (8 * a) for a, v in enumerate(d))
    d15_min = 0 if low >= 0 else 1
    d15_max = min((fr.p - 1 - low) >> 120, 127)
    d15 = d15_max if h[15][u] * s > 0 else d15_min
    x = low + (d15 << 120)
    assert 0 <= x < fr.p
    return x


def pair_sums(h, x):
    """The test's own integer model: what one (T, x) pair adds to each of the 16 accumulators,
    Y_v = sum_a h[a][v] d_a(x)."""
    d = FR.balanced_digits(x)
    return [sum(h[a][v] * d[a] for a in range(16)) for v in range(16)]
