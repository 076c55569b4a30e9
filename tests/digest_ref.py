"""The yardstick of the non-BLAKE3 digests: leaves, Merkle trees and paths of an lcpc-2d commitment
with D substituted (lcpc-2d/src/lib.rs:736-815), over Python's hashlib.  TEST INFRASTRUCTURE ONLY.

hashlib has SHA-256 and SHA3-256; Keccak-256 (the pre-standard padding byte 0x01) comes from the
plain-Python Keccak-f[1600] sponge below, which test_digest_ref.py pins to hashlib.sha3_256 (pad
0x06) and to the published Keccak-256 vectors.  BLAKE3 is pyref.blake3 (small inputs only: slow).
"""
from __future__ import annotations

import hashlib

import numpy as np

import pyref

BLAKE3, SHA256, SHA3_256, KECCAK256 = 0, 1, 2, 3
NAMES = {BLAKE3: "BLAKE3", SHA256: "SHA-256", SHA3_256: "SHA3-256", KECCAK256: "Keccak-256"}

_M64 = (1 << 64) - 1
_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B,
       0x0000000080000001, 0x8000000080008081, 0x8000000000008009, 0x000000000000008A, 0x0000000000000088,
       0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B, 0x8000000000008089,
       0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A,
       0x8000000080008081, 0x8000000000008080, 0x0000000080000001, 0x8000000080008008]


def _rho_offsets():
    # FIPS 202 3.2.2: (x, y) = (1, 0); for t in 0..23: r[x][y] = (t+1)(t+2)/2; (x, y) = (y, 2x + 3y)
    r = [0] * 25
    x, y = 1, 0
    for t in range(24):
        r[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


_ROT = _rho_offsets()


def _rotl(v, n: int):
    """rotate a lane left: a Python int, or a numpy uint64 array of lanes (one per message)"""
    if n == 0:
        return v
    if isinstance(v, np.ndarray):
        return (v << np.uint64(n)) | (v >> np.uint64(64 - n))
    return ((v << n) | (v >> (64 - n))) & _M64


def keccak_f1600(a):
    """Keccak-f[1600] on 25 lanes a[x + 5 y] (FIPS 202 3.2-3.4), in place.  A lane is a Python int,
    or a numpy uint64 array: the same permutation on many independent states at once."""
    vec = isinstance(a[0], np.ndarray)
    for rc in _RC:
        if vec:
            rc = np.uint64(rc)
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        for x in range(5):
            d = c[(x + 4) % 5] ^ _rotl(c[(x + 1) % 5], 1)
            for y in range(5):
                a[x + 5 * y] ^= d
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = _rotl(a[x + 5 * y], _ROT[x + 5 * y])
        for y in range(5):
            for x in range(5):
                nb = ~b[(x + 1) % 5 + 5 * y] if vec else ~b[(x + 1) % 5 + 5 * y] & _M64
                a[x + 5 * y] = b[x + 5 * y] ^ (nb & b[(x + 2) % 5 + 5 * y])
        a[0] = a[0] ^ rc
    return a


def keccak_sponge256(data: bytes, pad: int) -> bytes:
    """32-byte output of the rate-136 sponge; pad = 0x06: SHA3-256, 0x01: Keccak-256."""
    rate = 136
    msg = bytearray(data)
    msg.append(pad)
    msg += b"\0" * (-len(msg) % rate)
    msg[-1] |= 0x80
    a = [0] * 25
    for off in range(0, len(msg), rate):
        for i in range(rate // 8):
            a[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        keccak_f1600(a)
    return b"".join(a[i].to_bytes(8, "little") for i in range(4))


def keccak_sponge256_many(msgs, pad: int) -> list:
    """keccak_sponge256 of messages of one common length, the permutation run on all of them at
    once (numpy lanes): the same function, fast enough for a tree level or a row of leaves"""
    if not msgs:
        return []
    rate, n = 136, len(msgs[0])
    assert all(len(m) == n for m in msgs)
    padded = n + 1 + (-(n + 1) % rate)
    buf = np.zeros((len(msgs), padded), np.uint8)
    if n:
        buf[:, :n] = np.frombuffer(b"".join(msgs), np.uint8).reshape(len(msgs), n)
    buf[:, n] = pad
    buf[:, -1] |= 0x80
    lanes = buf.view("<u8").astype(np.uint64)  # (messages, padded / 8)
    a = [np.zeros(len(msgs), np.uint64) for _ in range(25)]
    for off in range(0, padded // 8, rate // 8):
        for i in range(rate // 8):
            a[i] = a[i] ^ lanes[:, off + i]
        keccak_f1600(a)
    out = np.stack(a[:4], axis=1).astype("<u8").tobytes()
    return [out[32 * i:32 * i + 32] for i in range(len(msgs))]


def digest_many(d: int, msgs) -> list:
    """digest(d, m) for every m of msgs (all of one length)"""
    msgs = list(msgs)
    if d == KECCAK256:
        return keccak_sponge256_many(msgs, 0x01)
    return [digest(d, m) for m in msgs]


def digest(d: int, data: bytes) -> bytes:
    if d == SHA256:
        return hashlib.sha256(data).digest()
    if d == SHA3_256:
        return hashlib.sha3_256(data).digest()
    if d == KECCAK256:
        return keccak_sponge256(data, 0x01)
    if d == BLAKE3:
        return pyref.blake3(data)
    raise ValueError(f"digest {d}")


def column_bytes(field: int, column_montgomery_limbs) -> bytes:
    """to_repr of every element of a column given as (n_rows, limbs) Montgomery u64 limbs"""
    f = pyref.Field(field)
    col = np.asarray(column_montgomery_limbs, dtype=np.uint64).reshape(-1, f.nl)
    r_inv = f.from_mont(1)  # (pyref.Field.from_mont(x) = x R^-1 mod p, the inverse taken once)
    out = []
    for row in col:
        mont = int.from_bytes(row.astype("<u8").tobytes(), "little")
        out.append(f.repr_bytes(mont * r_inv % f.p))
    return b"".join(out)


def leaf(d: int, field: int, column_montgomery_limbs) -> bytes:
    """hash_columns' digest of one column (:736-775): D(32 zero bytes || repr of each element)"""
    return digest(d, bytes(32) + column_bytes(field, column_montgomery_limbs))


def tree(d: int, leaves) -> list:
    """merkle_tree (:777-815): [leaves | level 1 | ... | root] as a list of 32-byte digests"""
    nodes = [bytes(x) for x in leaves]
    assert nodes and len(nodes) & (len(nodes) - 1) == 0
    lo, n = 0, len(nodes)
    while n > 1:
        nodes += digest_many(d, [nodes[lo + 2 * i] + nodes[lo + 2 * i + 1] for i in range(n // 2)])
        lo += n
        n //= 2
    return nodes


def path(tree_nodes: list, i: int) -> list:
    """open_column's path of leaf i (:818-855): the sibling at every level below the root"""
    n = (len(tree_nodes) + 1) // 2
    out, lo = [], 0
    while n > 1:
        out.append(tree_nodes[lo + (i ^ 1)])
        lo += n
        n //= 2
        i >>= 1
    return out


def commit_tree(d: int, field: int, comm, n_rows: int, n_cols: int) -> list:
    """the whole tree of a commitment from its row-major codeword comm (n_rows * n_cols, limbs)"""
    nl = pyref.Field(field).nl
    m = np.asarray(comm, dtype=np.uint64).reshape(n_rows, n_cols, nl)
    np2 = 1
    while np2 < n_cols:
        np2 *= 2
    leaves = digest_many(d, [bytes(32) + column_bytes(field, m[:, j]) for j in range(n_cols)])
    return tree(d, leaves + [bytes(32)] * (np2 - n_cols))


def mont_limbs(field: int, canonical: int):
    """u64 limbs of the Montgomery form of a canonical value"""
    f = pyref.Field(field)
    m = f.to_mont(canonical % f.p)
    return [(m >> (64 * i)) & _M64 for i in range(f.nl)]
