"""The Python yardstick of the non-BLAKE3 digests (tests/digest_ref.py) against hashlib and the
published Keccak-256 vectors, and lcpc_digest_name.  No GPU."""
import hashlib

import digest_ref as R


def test_sponge_pad06_is_sha3_256_on_every_length_to_300():
    data = bytes((7 * i + 3) & 0xFF for i in range(300))
    for n in range(301):
        assert R.keccak_sponge256(data[:n], 0x06) == hashlib.sha3_256(data[:n]).digest(), n


def test_sponge_pad01_is_keccak256():
    assert R.keccak_sponge256(b"", 0x01).hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert R.keccak_sponge256(b"abc", 0x01).hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert R.digest(R.KECCAK256, b"abc") == R.keccak_sponge256(b"abc", 0x01)


def test_vectorised_sponge_is_the_plain_one():
    data = bytes((11 * i + 1) & 0xFF for i in range(700))
    for n in (0, 1, 64, 135, 136, 137, 271, 272, 300):
        msgs = [data[k:k + n] for k in range(5)]
        for pad in (0x01, 0x06):
            assert R.keccak_sponge256_many(msgs, pad) == [R.keccak_sponge256(m, pad) for m in msgs], (n, pad)
    assert R.digest_many(R.SHA256, [b"a", b"b"]) == [hashlib.sha256(b"a").digest(), hashlib.sha256(b"b").digest()]


def test_column_bytes_is_pyref_repr():
    import pyref
    for fid in range(5):
        f = pyref.Field(fid)
        vals = [0, 1, f.p - 1, 0x0123456789ABCDEF % f.p]
        col = [R.mont_limbs(fid, v) for v in vals]
        assert R.column_bytes(fid, col) == b"".join(f.repr_bytes(f.from_mont(f.to_mont(v))) for v in vals)
        assert R.leaf(R.SHA256, fid, col) == hashlib.sha256(bytes(32) + R.column_bytes(fid, col)).digest()


def test_tree_and_path_shapes():
    leaves = [bytes([i]) * 32 for i in range(8)]
    t = R.tree(R.SHA256, leaves)
    assert len(t) == 15 and t[:8] == leaves
    assert t[8] == hashlib.sha256(leaves[0] + leaves[1]).digest()
    assert t[14] == hashlib.sha256(t[12] + t[13]).digest()
    p = R.path(t, 5)
    assert p == [leaves[4], t[8 + 3], t[12]]
    # walking the path as verify_column_path does (:985-1012) reaches the root
    h, i = leaves[5], 5
    for sib in p:
        h = hashlib.sha256(sib + h if i & 1 else h + sib).digest()
        i >>= 1
    assert h == t[-1]


def test_leaf_prefix_and_repr_order():
    # Ft253_192's repr is big-endian, the others' little-endian; 32 zero bytes lead the message
    one = R.mont_limbs(4, 1)
    assert R.leaf(R.SHA256, 4, [one]) == hashlib.sha256(bytes(32) + bytes(31) + b"\x01").digest()
    one = R.mont_limbs(1, 1)
    assert R.leaf(R.SHA3_256, 1, [one]) == hashlib.sha3_256(bytes(32) + b"\x01" + bytes(15)).digest()


def test_digest_name():
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import _native as N
    assert (L.BLAKE3, L.SHA256, L.SHA3_256, L.KECCAK256) == (0, 1, 2, 3)
    lib = N.load()
    assert [lib.lcpc_digest_name(d) for d in range(4)] == [b"BLAKE3", b"SHA-256", b"SHA3-256", b"Keccak-256"]
    assert lib.lcpc_digest_name(4) is None and lib.lcpc_digest_name(-1) is None
    assert [L.digest_name(d) for d in range(4)] == [R.NAMES[d] for d in range(4)]
    assert L.digest_name(17) is None
