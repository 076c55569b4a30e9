"""Big-integer reference for the primitives of csrc/field.hpp and the Ft127 digit recombination
of csrc/collapse_mfma.hpp, and the deterministic operand pool the GPU comparison runs over.
TEST INFRASTRUCTURE ONLY: Python integers, built on pyref.Field, nothing shared with the kernels.

Words are 32 bits, N per element, R = 2^(32 N).  Every field here has p = 1 mod 2^32, so
-p^-1 mod 2^32 = 0xffffffff.

    redc(T) = (T + ((T mod R) (-p^-1 mod R) mod R) p) / R          (no final subtraction)

The pool is where the comparison gets its strength: a carry fold dropped where it was needed
shows only when a column of the product scanning passes 2^64, which uniform random limbs do
with probability about 2^-32 per multiply-add.  So the pool holds the named edge values of each
domain, values whose limbs come from a small alphabet weighted towards 0xffffffff, and operand
pairs aimed at the quotient words m_k (all ones, or zero).
"""
from __future__ import annotations

import functools
import random

import numpy as np

import pyref

M32 = 0xFFFFFFFF
FIDS = [0, 1, 2, 3, 4]
POW_EXPONENTS = [0, 1, 2, 3, 1 << 32, (1 << 64) - 1]
N_ALPHABET_VALUES = 288  # with about 30 named values: about 10^5 pairs per binary op, 0.3 s of reference
DOT_TUPLES = 4096


class FieldRef:
    def __init__(self, fid: int):
        self.fid = fid
        self.f = pyref.Field(fid)
        self.p = self.f.p
        self.nl = self.f.nl  # u64 limbs
        self.N = 2 * self.nl  # u32 words
        self.R = self.f.R
        self.P = [(self.p >> (32 * i)) & M32 for i in range(self.N)]
        self.NP = (-pow(self.p, -1, self.R)) % self.R
        self.Rinv = pow(self.R, -1, self.p)
        self.dot_kmax = (1 << 32) // (self.P[-1] + 1)  # fe_dot_kmax: K p < R from the top word

    # ---- Montgomery reduction, closed form and word by word
    def redc(self, T: int) -> int:
        return (T + ((T % self.R) * self.NP % self.R) * self.p) // self.R

    def redc_words(self, T: int):
        """The same value word-serially, with the quotient words m_0 .. m_(N-1)."""
        ms = []
        for _ in range(self.N):
            m = (-T) & M32  # -p^-1 = -1 mod 2^32
            ms.append(m)
            T = (T + m * self.p) >> 32
        return T, ms

    # ---- expected raw output words of every op, as one integer per output
    def expected(self, op: str, a, b=None, k: int = 1):
        p, R = self.p, self.R
        if op == "add":
            return [(x + y) % p for x, y in zip(a, b)]
        if op == "sub":
            return [(x - y) % p for x, y in zip(a, b)]
        if op == "add_2p":
            return [x + y - (2 * p if x + y >= 2 * p else 0) for x, y in zip(a, b)]
        if op == "sub_2p":
            return [x - y + (2 * p if x < y else 0) for x, y in zip(a, b)]
        if op == "reduce_2p":
            return [x % p for x in a]
        if op == "sub_lazy":
            return [(x - y + p) % R for x, y in zip(a, b)]
        if op == "mul_sub_lazy":
            return [self.redc(((a[2 * i] - a[2 * i + 1]) % p) * y) % p for i, y in enumerate(b)]
        if op in ("mul", "mul_cios"):
            return [x * y * self.Rinv % p for x, y in zip(a, b)]
        if op == "sqr":
            return [x * x * self.Rinv % p for x in a]
        if op == "mul_lazy":
            return [self.redc(x * y) for x, y in zip(a, b)]
        if op == "dot":
            return [sum(a[i + q] * b[i + q] for q in range(k)) * self.Rinv % p for i in range(0, len(a), k)]
        if op == "from_mont":
            return [x * self.Rinv % p for x in a]
        if op == "from_mont_generic":  # redc exactly: equals x R^-1 mod p for x < p, may be p for x >= p
            return [self.redc(x) for x in a]
        if op == "to_mont":
            return [x * R % p for x in a]
        if op == "repr_words":
            return [int.from_bytes(self.f.repr_bytes(x * self.Rinv % p), "little") for x in a]
        if op == "canon_repr_words":
            return [int.from_bytes(self.f.repr_bytes(x), "little") for x in a]
        if op == "is_canonical":
            return [1 if x < p else 0 for x in a]
        if op == "pow":  # Montgomery in, Montgomery out: (a / R)^e R
            return [pow(x * self.Rinv, e, p) * R % p for x, e in zip(a, b)]
        if op == "balanced_digits":
            return [int.from_bytes(bytes(d & 0xFF for d in balanced_digits(x)), "little") for x in a]
        raise KeyError(op)

    # ---- arrays
    def to_array(self, vals) -> np.ndarray:
        nb = 8 * self.nl
        return np.frombuffer(b"".join(v.to_bytes(nb, "little") for v in vals), dtype="<u8").reshape(-1, self.nl).copy()

    def from_array(self, arr) -> list:
        nb = 8 * self.nl
        raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
        return [int.from_bytes(raw[i:i + nb], "little") for i in range(0, len(raw), nb)]


@functools.lru_cache(maxsize=None)
def field_ref(fid: int) -> FieldRef:
    """One FieldRef per field: the pool and the quotient-word search are cached on it (their results
    are shared: do not modify them)."""
    return FieldRef(fid)


def balanced_digits(x: int):
    """16 digits in [-128, 128) with sum d_a 2^(8a) = x (x below 2^127 - 2^120)."""
    ds = []
    for _ in range(16):
        d = ((x & 0xFF) ^ 0x80) - 0x80
        ds.append(d)
        x = (x - d) >> 8
    assert x == 0
    return ds


def recombine_expected(fr: FieldRef, rows):
    """(sum_u Y_u 2^(8u)) R^-1 mod p per row of 16 accumulators."""
    return [sum(int(y) << (8 * u) for u, y in enumerate(row)) * fr.Rinv % fr.p for row in rows]


# ---------------------------------------------------------------- the operand pool
DOMAINS = ("p", "2p", "R")


def _bound(fr: FieldRef, domain: str) -> int:
    return {"p": fr.p, "2p": 2 * fr.p, "R": fr.R}[domain]


def named_values(fr: FieldRef, domain: str):
    p, R, N = fr.p, fr.R, fr.N
    vals = [0, 1, 2, p - 1, p - 2, p - (1 << 32), (p + 1) // 2, (p - 1) // 2, R % p, R * R % p]
    for k in range(1, N):
        vals += [1 << (32 * k), (1 << (32 * k)) - 1]
    vals.append((1 << (32 * N)) - 1)  # the last limb boundary: R - 1, kept only by the R domain
    if domain in ("2p", "R"):
        vals += [p, p + 1, 2 * p - 1, 2 * p - 2]
    if domain == "R":
        vals += [R - 1]
        # equal to p in every limb above i, off by one in limb i: the comparison is decided at
        # limb i, whatever lies below (p's own limbs, and limbs that pull the other way)
        for i in range(N):
            high = (p >> (32 * (i + 1))) << (32 * (i + 1))
            below = (1 << (32 * i)) - 1
            if fr.P[i] > 0:
                vals += [high | ((fr.P[i] - 1) << (32 * i)) | (p & below), high | ((fr.P[i] - 1) << (32 * i)) | below]
            if fr.P[i] < M32:
                vals += [high | ((fr.P[i] + 1) << (32 * i)) | (p & below), high | ((fr.P[i] + 1) << (32 * i))]
    bound = _bound(fr, domain)
    return _dedup(v for v in vals if 0 <= v < bound)


def limb_alphabet(fr: FieldRef, i: int, rng: random.Random):
    return [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, fr.P[i], (fr.P[i] + 1) & M32, (fr.P[i] - 1) & M32,
            rng.getrandbits(32)]


def _draw_limb(fr, i, rng):
    """0xffffffff with weight 1/2, else one of the other letters."""
    if rng.random() < 0.5:
        return M32
    return rng.choice(limb_alphabet(fr, i, rng))


def _into_range(v: int, fr: FieldRef, bound: int) -> int:
    while v >= bound:
        v -= fr.p
    return v


def alphabet_values(fr: FieldRef, domain: str, count: int = N_ALPHABET_VALUES):
    bound = _bound(fr, domain)
    top = (bound - 1) >> (32 * (fr.N - 1))  # the bound's top limb (R: 0xffffffff)
    rng = random.Random(0x1CDC0000 + 16 * fr.fid + DOMAINS.index(domain))
    vals = []
    if fr.N == 2:  # the full cross product of the alphabet
        lows = _dedup(limb_alphabet(fr, 0, rng) + [M32])
        highs = _dedup(limb_alphabet(fr, 1, rng) + [M32] + [max(top - j, 0) for j in range(8)])
        for lo in lows:
            for hi in highs:
                vals.append(_into_range(lo | (hi << 32), fr, bound))
        return _dedup(vals)
    for n in range(count):
        v = 0
        for i in range(fr.N - 1):
            v |= _draw_limb(fr, i, rng) << (32 * i)
        v |= max(top - (n % 8), 0) << (32 * (fr.N - 1))
        vals.append(_into_range(v, fr, bound))
    return _dedup(vals)


@functools.lru_cache(maxsize=None)
def pool(fr: FieldRef, domain: str):
    return _dedup(named_values(fr, domain) + alphabet_values(fr, domain))


def _dedup(vals):
    seen, out = set(), []
    for v in vals:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _below_p_with_low(fr: FieldRef, low: int, rng: random.Random) -> int:
    """A value < p with the given low word: alphabet limbs above it, the top limb below p's."""
    v = low
    for i in range(1, fr.N - 1):
        v |= _draw_limb(fr, i, rng) << (32 * i)
    return v | ((fr.P[-1] - 1 - rng.randrange(8)) << (32 * (fr.N - 1)))


@functools.lru_cache(maxsize=None)
def quotient_pairs(fr: FieldRef):
    """Operand pairs (a, b), both < p, aimed at the quotient words of the product a b:
      "inv":  a_0 b_0 = 1 mod 2^32, so m_0 = 0xffffffff (a_0 = b_0 = 0xffffffff included);
      "zero": a_0 b_0 = 0 mod 2^32, so m_0 = 0;
      "ones": every m_k = 0xffffffff, i.e. a b = p mod R: b = p a^-1 mod R for odd a, kept when it
              is < p, and confirmed with the word-serial reduction.  "ones_words" is the number
              of all-ones quotient words of the first such pair (N when the search succeeded)."""
    rng = random.Random(0x51D0000 + fr.fid)
    inv, zero, ones = [], [], []
    for a0 in [M32, 1, 3, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFD] + [rng.getrandbits(32) | 1 for _ in range(10)]:
        b0 = pow(a0, -1, 1 << 32)
        for _ in range(4):
            inv.append((_below_p_with_low(fr, a0, rng), _below_p_with_low(fr, b0, rng)))
    for a0, b0 in [(0, 0), (0, M32), (M32, 0), (0x10000, 0x10000), (0x80000000, 2), (0x80000000, 0xFFFFFFFE),
                   (0xFFFF0000, 0xFFFF0000)]:
        for _ in range(4):
            zero.append((_below_p_with_low(fr, a0, rng), _below_p_with_low(fr, b0, rng)))
    best = (-1, None)
    for _ in range(4000):
        a = _below_p_with_low(fr, _draw_limb(fr, 0, rng) | 1, rng)
        b = fr.p * pow(a, -1, fr.R) % fr.R
        if b >= fr.p:
            continue
        n_ones = sum(m == M32 for m in fr.redc_words(a * b)[1])
        if n_ones > best[0]:
            best = (n_ones, (a, b))
        if n_ones == fr.N:
            ones.append((a, b))
            if len(ones) == 8:
                break
    if not ones:
        ones.append(best[1])
    return {"inv": inv, "zero": zero, "ones": ones,
            "ones_words": sum(m == M32 for m in fr.redc_words(ones[0][0] * ones[0][1])[1])}


def cross(xs, ys):
    """The cross product as two parallel operand lists."""
    return [x for x in xs for _ in ys], [y for _ in xs for y in ys]


def mul_pairs(fr: FieldRef, a_domain: str = "p"):
    """Operands of a multiplicative op: pool(a_domain) x pool(p) and the quotient-word targets."""
    a, b = cross(pool(fr, a_domain), pool(fr, "p"))
    q = quotient_pairs(fr)
    for x, y in q["inv"] + q["zero"] + q["ones"]:
        a.append(x)
        b.append(y)
        if a_domain == "2p":  # a + p as well: the upper half of the lazy domain, other quotient words
            a.append(x + fr.p)
            b.append(y)
    return a, b


def dot_tuples(fr: FieldRef, k: int, count: int = DOT_TUPLES):
    """count k-tuples drawn from the pool, then the tuple that decides the cap K p < R: every
    a_q = b_q = p - 1, the largest sum K (p - 1)^2."""
    rng = random.Random(0xD07 + 64 * fr.fid + k)
    pl = pool(fr, "p")
    q = quotient_pairs(fr)
    pairs = q["inv"] + q["ones"]  # every fourth tuple is made of quotient-word target pairs
    a, b = [], []
    for n in range(count):
        for _ in range(k):
            if n % 4 == 3:
                x, y = rng.choice(pairs)
            else:
                x, y = rng.choice(pl), rng.choice(pl)
            a.append(x)
            b.append(y)
    a += [fr.p - 1] * k
    b += [fr.p - 1] * k
    return a, b


# ---------------------------------------------------------------- the comparison's cases
# case name -> (op of lcpc_selftest_field_op, k); the operands come from operands()
def case_names(fr: FieldRef):
    names = ["add", "sub", "add_2p", "sub_2p", "reduce_2p", "sub_lazy", "mul_sub_lazy", "mul", "mul_a_below_2p",
             "mul_cios", "sqr", "mul_lazy", "from_mont", "from_mont_generic", "to_mont", "repr_words",
             "canon_repr_words", "is_canonical", "pow"]
    names += [f"dot{k}" for k in range(1, fr.dot_kmax + 1)]
    if fr.fid == 1:
        names += ["from_mont_generic_any", "balanced_digits"]
    return names


def case_op(name: str):
    if name.startswith("dot"):
        return "dot", int(name[3:])
    return {"mul_a_below_2p": "mul", "from_mont_generic_any": "from_mont_generic"}.get(name, name), 1


def operands(fr: FieldRef, name: str):
    """(a, b) of a case as lists of integers in the op's domain (b None for a unary op)."""
    pp, p2 = pool(fr, "p"), pool(fr, "2p")
    if name in ("add", "sub", "sub_lazy"):
        return cross(pp, pp)
    if name in ("add_2p", "sub_2p"):
        return cross(p2, p2)
    if name == "reduce_2p":
        return p2, None
    if name == "mul_sub_lazy":
        rng = random.Random(0x5B1A + fr.fid)
        small = _dedup(named_values(fr, "p") + alphabet_values(fr, "p")[:40])
        a, b = [], []
        for a0 in small:
            for a1 in small:
                for _ in range(5):
                    a += [a0, a1]
                    b.append(rng.choice(pp))
        return a, b
    if name in ("mul", "mul_cios"):
        return mul_pairs(fr, "p")
    if name in ("mul_a_below_2p", "mul_lazy"):
        return mul_pairs(fr, "2p")
    if name == "sqr":
        return _dedup(pp + [x for x, _ in quotient_pairs(fr)["inv"]]), None
    if name.startswith("dot"):
        return dot_tuples(fr, int(name[3:]))
    if name in ("from_mont", "from_mont_generic", "to_mont", "repr_words", "canon_repr_words", "balanced_digits"):
        return pp, None
    if name in ("is_canonical", "from_mont_generic_any"):
        return pool(fr, "R"), None
    if name == "pow":
        return cross(pp, POW_EXPONENTS)
    raise KeyError(name)
