"""Pure-Python reference of the batched stored-file audit's arithmetic (big integers), used only by
tests.  TEST INFRASTRUCTURE ONLY.

  left_mul        out[c] = sum_r left[r] M[r][c] / R mod p over the 7-byte image (k_left_mul_bytes' rule)
  h_digits        the matrix-core kernel's left operand: h[a][u], the 8 balanced base-256 digits of
                  left 2^(8a) mod p, a < 7
  accumulators    Y[u] = sum_(r, a) h[r][a][u] (b_a(r) - 128) for one column of file elements
  recombine       (sum_u Y[u] 2^(8u)) / R mod p, what recombine_redc63 returns
  same_sign_rows  left words and an image column that drive one accumulator with products of one sign
"""
from __future__ import annotations

import random

from pyref import Field
from update_ref import pack7

F63 = Field(0)
P, R = F63.p, F63.R
RINV = pow(R, -1, P)
C128 = 0x0080808080808080                  # sum_a 128 2^(8a), a < 7
MAX_SPLIT_ROWS = 512                       # pos_eval_mfma.hpp
Y_BOUND = 1 << 26                          # the bound the kernel documents for |Y[u]|
Y_MAX = MAX_SPLIT_ROWS * 7 * 128 * 128     # what 512 rows of 7 digit products can reach (2^25.81)
BALANCE = 0x8080808080808080
TOP_DIGIT_MAX = P >> 56                    # position 7 holds the top byte of a value below p: 0 .. 0x46


def reach(u: int) -> int:
    """what |Y[u]| can reach over a 512-row split: Y_MAX, less at position 7 whose digits are small"""
    return MAX_SPLIT_ROWS * 7 * TOP_DIGIT_MAX * 128 if u == 7 else Y_MAX


def left_mul(data: bytes, pre: int, left) -> list:
    el = pack7(data)
    n_rows = -(-len(el) // pre)
    assert len(left) == n_rows
    el += [0] * (n_rows * pre - len(el))
    return [sum(left[r] * el[r * pre + c] for r in range(n_rows)) * RINV % P for c in range(pre)]


def h_digits(left_word: int) -> list:
    out = []
    for a in range(7):
        v = (left_word << (8 * a)) % P + BALANCE
        assert v < 1 << 64, "p < 2^63 - 2^56: no carry out"
        out.append([((v >> (8 * u)) & 0xff) - 128 for u in range(8)])
    return out


def accumulators(left, elems) -> list:
    """Y[0..7] of one column: elems[r] is the raw 56-bit file element of row r"""
    Y = [0] * 8
    for lw, e in zip(left, elems):
        h = h_digits(lw)
        for a in range(7):
            d = ((e >> (8 * a)) & 0xff) - 128
            for u in range(8):
                Y[u] += h[a][u] * d
    return Y


def recombine(Y) -> int:
    return sum(y << (8 * u) for u, y in enumerate(Y)) * RINV % P


def column_value(left, elems) -> int:
    """the kernel's route to one output: recombine the accumulators, add the C128 term"""
    return (recombine(accumulators(left, elems)) + sum(left) % P * C128 * RINV) % P


def same_sign_rows(u: int, n_rows: int, seed: int, tries: int = 32, mirror: bool = False):
    """(left words, elements): every row's word is the one of `tries` random words whose digits at
    position u are largest in sum of magnitudes, and the element's byte a is 0xff (digit 127) where
    h[a][u] > 0 and 0x00 (digit -128) elsewhere (mirror: the other way round), so every product in
    accumulator u has the same sign."""
    rng = random.Random(seed)
    left, elems = [], []
    for _ in range(n_rows):
        best, best_h = None, None
        for _ in range(tries):
            w = rng.randrange(P)
            h = h_digits(w)
            s = sum(abs(h[a][u]) for a in range(7))
            if best is None or s > best:
                best, best_w, best_h = s, w, h
        left.append(best_w)
        elems.append(sum((0xff if (best_h[a][u] > 0) != mirror else 0) << (8 * a) for a in range(7)))
    return left, elems
