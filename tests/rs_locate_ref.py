"""Python-integer restatement of Reed-Solomon error location (tests only): syndromes, inversion-free
Berlekamp-Massey, roots by evaluating the connection polynomial at pos.rs_domain_points.

Built on the oracle's modulus, conversions and transforms only.  A row of len evaluations y_c of a
polynomial of degree < n_per_row at the points x_c, the positions E erased, the positions Err wrong:

  g_c = y_c L0(x_c), L0(x) = prod_{j in E} (x - x_j), 0 at E          (the erased y_c are never read)
  p   = ifft_oi(g)                     coefficients of f L0 plus the transform of the masked errors
  S_i = p[k' + i], k' = n_per_row + |E|, i < N = len - k'             power sums of the wrong positions
  C   = the shortest recurrence of S (Berlekamp-Massey, no inversion): roots = {x_c : c in Err}

The outcome per row is (status, L, positions): 0 a codeword, 1 located, 2 not locatable (2 L > N,
C_L = 0, the number of roots is not L, a root on an erased position, or L > max_errors).
"""
import numpy as np

import oracle_ffi as O


def berlekamp_massey(S, p):
    """(C, L): C[0..L] with sum_j C[j] S[i - j] = 0 for L <= i < len(S), L minimal; C up to a scalar."""
    C, B, L, b, m = [1], [1], 0, 1, 1
    for i in range(len(S)):
        d = 0
        for j in range(min(L, len(C) - 1) + 1):
            d += C[j] * S[i - j]
        d %= p
        if d == 0:
            m += 1
            continue
        T = C
        n = max(len(C), len(B) + m)
        new = [(b * (C[j] if j < len(C) else 0)) % p for j in range(n)]
        for j, bj in enumerate(B):
            new[j + m] = (new[j + m] - d * bj) % p
        C = new
        if 2 * L <= i:
            L, B, b, m = i + 1 - L, T, d, 1
        else:
            m += 1
    C = (C + [0] * (L + 1))[:L + 1]
    return C, L


class Locator:
    """The per-(field, len, n_per_row, erased) tables, shared by the rows of a batch."""

    def __init__(self, pos, fid, length, n_per_row, erased=(), max_errors=None, roots_by=None):
        self.fid, self.n, self.k = fid, length, n_per_row
        self.p = O.modulus(fid)
        self.nl = O.limbs(fid)
        self.erased = [int(e) for e in erased]
        self.points = O.from_mont(fid, pos.rs_domain_points(fid, length).reshape(-1))
        self.kp = n_per_row + len(self.erased)
        self.N = length - self.kp
        self.max_errors = max_errors
        # Horner at every point for short rows; the oracle's fft_io of C (the same evaluations: position
        # c of a codeword of f is f(points[c])) for long ones
        self.roots_by = roots_by or ("horner" if length <= 64 else "fft")
        ex = [self.points[j] for j in self.erased]
        self.l0 = []
        for c, x in enumerate(self.points):
            v = 1
            for xj in ex:
                v = v * (x - xj) % self.p
            self.l0.append(v)
        self.is_erased = [False] * length
        for j in self.erased:
            self.is_erased[j] = True

    def syndromes(self, row):
        """row: (len, limbs) Montgomery limbs.  The N syndromes as integers."""
        if self.N <= 0:
            return []
        keep = np.array(row, np.uint64).reshape(self.n, self.nl).copy()
        keep[self.erased] = 0                          # never read
        y = O.from_mont(self.fid, keep.reshape(-1))
        g = [0 if self.is_erased[c] else y[c] * self.l0[c] % self.p for c in range(self.n)]
        coeffs = O.from_mont(self.fid, O.ifft_oi(self.fid, O.to_mont(self.fid, g)))
        return coeffs[self.kp:]

    def evaluate(self, C):
        if self.roots_by == "horner":
            out = []
            for x in self.points:
                v = 0
                for cj in reversed(C):
                    v = (v * x + cj) % self.p
                out.append(v)
            return out
        return O.from_mont(self.fid, O.fft_io(self.fid, O.to_mont(self.fid, list(C) + [0] * (self.n - len(C)))))

    def locate(self, row):
        """(status, L, positions) of one row."""
        S = self.syndromes(row)
        if not any(S):
            return 0, 0, []
        C, L = berlekamp_massey(S, self.p)
        if 2 * L > self.N or C[L] == 0 or (self.max_errors is not None and L > self.max_errors):
            return 2, 0, []
        roots = [c for c, v in enumerate(self.evaluate(C)) if v == 0]
        if len(roots) != L or any(self.is_erased[c] for c in roots):
            return 2, 0, []
        return 1, L, roots


# ---------------------------------------------------------------- inputs shared by the tests
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
_codewords = {}


def codewords(fid, npr, length, n=130):
    """n codewords (n, len, limbs) of seeded random messages, computed once per shape; never modified."""
    key = (fid, npr, length, n)
    if key not in _codewords:
        nl = O.limbs(fid)
        msgs = O.random_coeffs(fid, n * npr, 0x10CA7E + 131 * fid + length).reshape(n, npr * nl)
        rows = np.zeros((n, length * nl), np.uint64)
        for r in range(n):
            row = np.zeros(length * nl, np.uint64)
            row[:npr * nl] = msgs[r]
            rows[r] = O.fft_io(fid, row)
        rows = rows.reshape(n, length, nl)
        rows.setflags(write=False)
        _codewords[key] = rows
    return _codewords[key]


def error_positions(avail, t, pattern, rng):
    """t of the positions `avail` (ascending): 0 the first ones (position 0 when nothing is erased), 1
    the last ones (len - 1), 2 a contiguous run in the middle, 3 a random set."""
    if t == 0:
        return []
    if pattern == 0:
        return list(avail[:t])
    if pattern == 1:
        return list(avail[-t:])
    if pattern == 2:
        lo = (len(avail) - t) // 2
        return list(avail[lo:lo + t])
    return sorted(int(c) for c in rng.choice(avail, size=t, replace=False))


def damage(fid, row, positions, erased, rng, plus_one=False):
    """A copy of the codeword row (len, limbs): every position in `positions` holds a different, fully
    reduced element (seeded random, or the codeword's value + 1), the erased ones all-ones limbs."""
    nl, p = O.limbs(fid), O.modulus(fid)
    out = np.array(row, np.uint64).copy()
    one = O.ints_from_limbs(O.to_mont(fid, [1]), nl)[0]
    for c in positions:
        old = O.ints_from_limbs(out[c], nl)[0]
        if plus_one:
            new = (old + one) % p
        else:
            new = int.from_bytes(rng.bytes(8 * nl), "little") % p
            if new == old:
                new = (new + 1) % p
        out[c] = O.limbs_from_ints([new], nl)
    out[list(erased)] = ONES
    return out
