"""Commitments, openings, proofs and verification under a digest chosen by the caller (lcpc_digest:
BLAKE3, SHA-256, SHA3-256, Keccak-256), on the GPU, against hashlib (tests/digest_ref.py).

The reference's LcCommit<D, E> leaves D free (lcpc-2d/src/lib.rs:174-191); its transcript absorbs no
digest (:1057, :1075-1077, :1096-1104), so under one transcript a proof differs between digests only
in its Merkle paths: everything else is pinned to the BLAKE3 proof, which the C oracle checks
elsewhere, and the hashes to hashlib.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import digest_ref as R
import pyref

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2, 3, 4]
NEW = [R.SHA256, R.SHA3_256, R.KECCAK256]
ALL = [R.BLAKE3] + NEW

# leaf shapes: the message is 32 + n_rows * {8, 16, 24, 32} bytes.  n_rows 1..9 reach every residue
# mod 64 a field can reach (56, where SHA-256's padding spills into another block: Ft63 at 3 rows,
# Ft191 at 1; 0, a padding-only block), 1..18 every residue mod 136 (0, the extra rate block, at
# 13 / 15 / 10 / 16 rows; 128, both padding bytes in the last lane, at 12 / 6); 67 rows run several
# periods of the unrolled absorb.  65 and 300 columns end in a partial wave.
LEAF_ROWS = list(range(1, 19)) + [67]
LEAF_COLS = [1, 2, 65, 300]
MAX_ROWS, MAX_COLS = 67, 300


@functools.lru_cache(maxsize=None)
def leaf_matrix(fid):
    """(MAX_ROWS, MAX_COLS, limbs) Montgomery elements -- random, with the extreme residues 0 and
    p - 1 sprinkled in -- and each column's repr bytes; a case takes the top-left corner."""
    f = pyref.Field(fid)
    rng = np.random.default_rng(1000 + fid)
    m = np.zeros((MAX_ROWS, MAX_COLS, f.nl), np.uint64)
    for r in range(MAX_ROWS):
        for c in range(MAX_COLS):
            k = (r * MAX_COLS + c) % 11
            v = 0 if k == 0 else f.p - 1 if k == 5 else int.from_bytes(rng.bytes(8 * f.nl), "little") % f.p
            m[r, c] = R.mont_limbs(fid, v)
    col_bytes = [R.column_bytes(fid, m[:, c]) for c in range(MAX_COLS)]
    return m, col_bytes


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("d", NEW)
def test_leaves(gpu, d, fid):
    m, col_bytes = leaf_matrix(fid)
    eb = 8 * pyref.Field(fid).nl
    for n_rows in LEAF_ROWS:
        for n_cols in LEAF_COLS:
            sub = np.ascontiguousarray(m[:n_rows, :n_cols])
            got = gpu.hash_columns(fid, sub, n_rows, n_cols, digest=d)
            want = R.digest_many(d, [bytes(32) + col_bytes[c][:n_rows * eb] for c in range(n_cols)])
            assert got == b"".join(want), (n_rows, n_cols)
            # (the messages above are digest_ref.leaf's: one column spelled out per shape)
            assert want[n_cols - 1] == R.leaf(d, fid, sub[:, n_cols - 1])


@pytest.mark.parametrize("fid", FIELDS)
def test_leaves_blake3_through_the_digest_entry(gpu, fid):
    """lcpc_hash_columns_d(BLAKE3) is lcpc_hash_columns, and the BLAKE3 of digest_ref"""
    from lcpc_proof_of_storage_amd import _native as N
    m, _ = leaf_matrix(fid)
    for n_rows, n_cols in [(1, 1), (9, 2), (18, 65), (67, 300)]:
        sub = np.ascontiguousarray(m[:n_rows, :n_cols])
        out = (C.c_uint8 * (32 * n_cols))()
        flat = sub.reshape(-1, sub.shape[2])
        assert N.load().lcpc_hash_columns_d(R.BLAKE3, fid, gpu.lcpc2d._p64(flat), n_rows, n_cols,
                                            C.cast(out, N.u8p)) == 0
        assert bytes(out) == gpu.hash_columns(fid, sub, n_rows, n_cols)
        assert bytes(out)[:32] == R.leaf(R.BLAKE3, fid, sub[:, 0])


@pytest.mark.parametrize("n_ins", [2, 4, 1024, 8192])
@pytest.mark.parametrize("d", NEW)
def test_merkle(gpu, d, n_ins):
    leaves = np.random.default_rng(n_ins).bytes(32 * n_ins)
    want = R.tree(d, [leaves[32 * i:32 * i + 32] for i in range(n_ins)])
    assert gpu.merkle_tree(leaves, digest=d) == b"".join(want[n_ins:])


# ---------------------------------------------------------------- commit / prove / verify
def _encoding(gpu, kind, fid, d, ndt=None):
    if kind == "sdig":
        enc = gpu.SdigEncoding.new(fid, 1 << 12, 0)  # SdigCode3: a column-major, non-power-of-two codeword
    elif ndt is None:
        enc = gpu.LigeroEncoding.new(fid, 1 << 12)
    else:
        ref = gpu.LigeroEncoding.new(fid, 1 << 12)
        enc = gpu.RsEncoding.new(fid, ref.n_per_row, ref.n_cols, 24, ndt)
    if d != R.BLAKE3:
        assert enc.set_digest(d) is enc
    assert enc.digest == d
    return enc


@functools.lru_cache(maxsize=None)
def _coeffs(fid):
    import lcpc_proof_of_storage_amd as L
    return L.field_random(fid, 1 << 12, 40 + fid)


@functools.lru_cache(maxsize=None)
def _blake3_commit(kind, fid):
    """the BLAKE3 commitment of a case, its codeword and the proof the others are pinned to"""
    import lcpc_proof_of_storage_amd as L
    enc = _encoding(L, kind, fid, R.BLAKE3)
    comm = L.LcCommit.commit(_coeffs(fid), enc)
    outer = L.field_random(fid, comm.get_n_rows(), 50 + fid)
    inner = L.field_random(fid, comm.get_n_per_row(), 60 + fid)
    root = comm.get_root()
    proof = comm.prove(outer, enc, _seeded(L, root))
    ev = proof.verify(root, outer, inner, enc, _seeded(L, root))
    return dict(enc=enc, comm=comm, codeword=comm.comm, outer=outer, inner=inner, root=root, proof=proof, ev=ev)


def _seeded(gpu, blake3_root):
    """one transcript for every digest: seeded as for the BLAKE3 proof of the polynomial"""
    tr = gpu.Transcript(b"test transcript")
    tr.append_message(b"polycommit", blake3_root)
    return tr


class _Forwarding:
    """a caller-owned transcript (CallerTranscript wraps it): merlin's methods onto a library one"""

    def __init__(self, tr):
        self.tr, self.calls = tr, 0

    def append_message(self, label, msg):
        self.calls += 1
        self.tr.append_message(label, msg)

    def challenge_bytes(self, label, n):
        self.calls += 1
        return self.tr.challenge_bytes(label, n)


CASES = [("ligero", f) for f in FIELDS] + [("sdig", 1)]


@functools.lru_cache(maxsize=None)
def _commit(kind, fid, d):
    import lcpc_proof_of_storage_amd as L
    b = _blake3_commit(kind, fid)
    enc = _encoding(L, kind, fid, d)
    comm = L.LcCommit.commit(_coeffs(fid), enc)
    tree = R.commit_tree(d, fid, b["codeword"], comm.get_n_rows(), comm.get_n_cols())
    return enc, comm, tree


@pytest.mark.parametrize("kind,fid", CASES)
@pytest.mark.parametrize("d", NEW)
def test_commit(gpu, d, kind, fid):
    b = _blake3_commit(kind, fid)
    enc, comm, tree = _commit(kind, fid, d)
    assert comm.digest == d and b["comm"].digest == R.BLAKE3
    assert np.array_equal(comm.comm, b["codeword"])
    if kind == "sdig":
        n_cols = comm.get_n_cols()
        assert n_cols & (n_cols - 1), "the SDIG case is there for the zero-digest padding"
    assert comm.hashes == b"".join(tree)
    assert comm.get_root() == tree[-1] != b["root"]
    comm.check(enc)


def _column_index(codeword, n_rows, n_cols, col):
    m = codeword.reshape(n_rows, n_cols, -1)
    hits = np.where((m == col[:, None, :]).all(axis=(0, 2)))[0]
    assert len(hits) == 1
    return int(hits[0])


def _pinned_to_blake3(gpu, pf, b, tree):
    """everything but the paths is the BLAKE3 proof's; every path is the reference tree's"""
    ref = b["proof"]
    assert np.array_equal(pf.p_eval, ref.p_eval)
    assert len(pf.p_random_vec) == len(ref.p_random_vec) > 0
    for x, y in zip(pf.p_random_vec, ref.p_random_vec):
        assert np.array_equal(x, y)
    cols, ref_cols = pf.columns, ref.columns
    assert len(cols) == len(ref_cols) > 0
    n_rows, n_cols = b["comm"].get_n_rows(), b["comm"].get_n_cols()
    for c, rc in zip(cols, ref_cols):
        assert np.array_equal(c.col, rc.col)
        i = _column_index(b["codeword"], n_rows, n_cols, c.col)
        assert c.path == R.path(tree, i)


@pytest.mark.parametrize("kind,fid", CASES)
@pytest.mark.parametrize("d", NEW)
def test_prove(gpu, d, kind, fid):
    b = _blake3_commit(kind, fid)
    enc, comm, tree = _commit(kind, fid, d)
    _pinned_to_blake3(gpu, comm.prove(b["outer"], enc, _seeded(gpu, b["root"])), b, tree)
    caller = _Forwarding(_seeded(gpu, b["root"]))
    _pinned_to_blake3(gpu, comm.prove(b["outer"], enc, caller), b, tree)
    assert caller.calls > 0


def test_prove_ops_entry_point(gpu):
    """lcpc_prove_ops / lcpc_verify_ops (the C ABI a shim binds) under SHA-256"""
    from lcpc_proof_of_storage_amd import _native as N
    lib = N.load()
    kind, fid, d = "ligero", 1, R.SHA256
    b = _blake3_commit(kind, fid)
    enc, comm, tree = _commit(kind, fid, d)
    target = _seeded(gpu, b["root"])

    def am(ctx, lp, ln, mp, mn):
        lib.lcpc_transcript_append_message(target._h, lp, ln, mp, mn)
        return 0

    def ch(ctx, lp, ln, dp, n):
        lib.lcpc_transcript_challenge_bytes(target._h, lp, ln, dp, n)
        return 0

    cbs = (N.TR_APPEND_FN(am), N.TR_APPEND_MANY_FN(), N.TR_CHALLENGE_FN(ch))
    ops = N.TranscriptOps(None, *cbs)
    o = gpu.lcpc2d._elems(b["outer"], fid)
    h = C.c_void_p()
    assert lib.lcpc_prove_ops(comm._h, gpu.lcpc2d._p64(o), o.shape[0], enc._h, C.byref(ops), C.byref(h)) == 0
    pf = gpu.LcEvalProof(h.value)
    _pinned_to_blake3(gpu, pf, b, tree)
    target = _seeded(gpu, b["root"])
    i = gpu.lcpc2d._elems(b["inner"], fid)
    ev = np.zeros(gpu.limbs(fid), np.uint64)
    rp = (C.c_uint8 * 32).from_buffer_copy(comm.get_root())
    assert lib.lcpc_verify_ops(rp, gpu.lcpc2d._p64(o), o.shape[0], gpu.lcpc2d._p64(i), i.shape[0], pf._h, enc._h,
                               C.byref(ops), gpu.lcpc2d._p64(ev)) == 0
    assert np.array_equal(ev, b["ev"].reshape(-1))
    # a BLAKE3 encoding over the same proof and root: the paths do not lead there
    target = _seeded(gpu, b["root"])
    assert lib.lcpc_verify_ops(rp, gpu.lcpc2d._p64(o), o.shape[0], gpu.lcpc2d._p64(i), i.shape[0], pf._h,
                               b["enc"]._h, C.byref(ops), gpu.lcpc2d._p64(ev)) == 11  # LCPC_VERIFIER_COLUMN_PATH


def _column_path_error(fn):
    with pytest.raises(Exception) as ei:
        fn()
    assert type(ei.value).__name__ == "VerifierError" and ei.value.code == 11, ei.value  # ColumnPath


@pytest.mark.parametrize("kind,fid", CASES)
@pytest.mark.parametrize("d", NEW)
def test_verify(gpu, d, kind, fid):
    b = _blake3_commit(kind, fid)
    enc, comm, tree = _commit(kind, fid, d)
    root, outer, inner = comm.get_root(), b["outer"], b["inner"]
    pf = comm.prove(outer, enc, _seeded(gpu, b["root"]))
    ev = pf.verify(root, outer, inner, enc, _seeded(gpu, b["root"]))
    assert np.array_equal(ev, b["ev"])
    # the verifier's encoding says which digest the root belongs to: any other one fails the paths
    for other in ALL:
        if other != d:
            e2 = _encoding(gpu, kind, fid, other)
            _column_path_error(lambda: pf.verify(root, outer, inner, e2, _seeded(gpu, b["root"])))
    # one path byte flipped
    cols = pf.columns
    k = len(cols) // 2
    p = list(cols[k].path)
    p[-1] = p[-1][:7] + bytes([p[-1][7] ^ 0x10]) + p[-1][8:]
    bad = [gpu.LcColumn(c.col, p if j == k else c.path) for j, c in enumerate(cols)]
    pf_bad = gpu.LcEvalProof.from_parts(fid, pf.n_cols, pf.p_eval, pf.p_random_vec, bad)
    _column_path_error(lambda: pf_bad.verify(root, outer, inner, enc, _seeded(gpu, b["root"])))


@pytest.mark.parametrize("fid", [0, 2, 4])
@pytest.mark.parametrize("d", NEW)
def test_verify_changed_column_element(gpu, d, fid):
    """One opened element changed with the evaluation checks kept satisfied trivially: no degree
    tests, and a zero in the outer tensor at the changed row, so that only the leaf (built into the
    root from the other value) can tell."""
    enc = _encoding(gpu, "ligero", fid, d, ndt=0)
    comm = gpu.LcCommit.commit(_coeffs(fid), enc)
    row = comm.get_n_rows() // 2
    outer = gpu.field_random(fid, comm.get_n_rows(), 70 + fid)
    outer[row] = 0
    inner = gpu.field_random(fid, comm.get_n_per_row(), 71 + fid)
    root = comm.get_root()
    pf = comm.prove(outer, enc, gpu.Transcript(b"changed"))
    pf.verify(root, outer, inner, enc, gpu.Transcript(b"changed"))
    cols = pf.columns
    k = len(cols) - 1
    col = cols[k].col.copy()
    col[row, 0] ^= np.uint64(1)
    bad = [gpu.LcColumn(col if j == k else c.col, c.path) for j, c in enumerate(cols)]
    pf_bad = gpu.LcEvalProof.from_parts(fid, pf.n_cols, pf.p_eval, pf.p_random_vec, bad)
    _column_path_error(lambda: pf_bad.verify(root, outer, inner, enc, gpu.Transcript(b"changed")))


# ---------------------------------------------------------------- boundary
@pytest.mark.parametrize("d", NEW)
def test_from_bincode_round_trip(gpu, d):
    kind, fid = "ligero", 1
    b = _blake3_commit(kind, fid)
    enc, comm, tree = _commit(kind, fid, d)
    data = comm.to_bincode()
    back = gpu.LcCommit.from_bincode(fid, data, digest=d)
    assert back.digest == d and back.to_bincode() == data and back.get_root() == tree[-1]
    _pinned_to_blake3(gpu, back.prove(b["outer"], enc, _seeded(gpu, b["root"])), b, tree)
    # the bytes do not say which digest: loaded as BLAKE3, the handle is a BLAKE3 commitment
    assert gpu.LcCommit.from_bincode(fid, data).digest == R.BLAKE3


def test_mismatched_digest_is_invalid_arg(gpu):
    kind, fid = "ligero", 0
    b = _blake3_commit(kind, fid)
    enc, comm, _ = _commit(kind, fid, R.KECCAK256)
    for c, e in [(comm, b["enc"]), (b["comm"], enc), (comm, _encoding(gpu, kind, fid, R.SHA3_256))]:
        with pytest.raises(gpu.LcpcError) as ei:
            c.prove(b["outer"], e, _seeded(gpu, b["root"]))
        assert ei.value.code == 30 and "digest" in str(ei.value)  # LCPC_ERR_INVALID_ARG
        with pytest.raises(gpu.LcpcError) as ei:
            c.check(e)
        assert ei.value.code == 30
    with pytest.raises(gpu.LcpcError) as ei:
        enc.set_digest(4)
    assert ei.value.code == 30 and enc.digest == R.KECCAK256


@pytest.mark.parametrize("d", NEW)
def test_verify_column_path_d(gpu, d):
    kind, fid = "ligero", 3
    _, comm, tree = _commit(kind, fid, d)
    root = comm.get_root()
    for i in (0, comm.get_n_cols() - 1, 37):
        col = comm.open_column(i)
        assert col.path == R.path(tree, i)
        assert gpu.verify_column_path(fid, col, i, root, digest=d)
        assert not gpu.verify_column_path(fid, col, i ^ 1, root, digest=d)
        assert not gpu.verify_column_path(fid, col, i, root)  # (the old name stays BLAKE3)
        for other in NEW:
            assert gpu.verify_column_path(fid, col, i, root, digest=other) == (other == d)


def test_blake3_only_entry_points_refuse_and_nothing_leaks(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    lib = N.load()
    fid = 0
    coeffs = _coeffs(fid)
    before = gpu.LcCommit.commit(coeffs, gpu.LigeroEncoding.new(fid, 1 << 12)).get_root()
    assert before == _blake3_commit("ligero", fid)["root"]
    image = np.arange(7 * 5000, dtype=np.uint64).astype(np.uint8)
    want = gpu.LcCommit.commit_pos_bytes(image, gpu.LigeroEncoding.new(fid, 5000)).get_root()
    for d in NEW:
        enc = gpu.LigeroEncoding.new(fid, 5000).set_digest(d)
        with pytest.raises(gpu.LcpcError) as ei:
            gpu.LcCommit.commit_pos_bytes(image, enc)
        assert ei.value.code == 34 and R.NAMES[d] in str(ei.value)  # LCPC_ERR_UNSUPPORTED, naming the digest
        h = C.c_void_p()
        rows = np.ascontiguousarray(coeffs[:enc.n_per_row])
        assert lib.lcpc_shard_new(enc._h, gpu.lcpc2d._p64(rows), 0, 1, 4, C.byref(h)) == 34
        assert R.NAMES[d].encode() in N.last_error().encode() and not h.value
        idx = np.zeros(1, np.uint64)
        out = np.zeros((4096, 1), np.uint64)
        assert lib.lcpc_pos_columns(enc._h, gpu.lcpc2d._p64(coeffs), coeffs.shape[0], gpu.lcpc2d._p64(idx), 1,
                                    gpu.lcpc2d._p64(out), None) == 34
    # BLAKE3 after all of the above: the roots it gave before
    assert gpu.LcCommit.commit_pos_bytes(image, gpu.LigeroEncoding.new(fid, 5000)).get_root() == want
    assert gpu.LcCommit.commit(coeffs, gpu.LigeroEncoding.new(fid, 1 << 12)).get_root() == before
    leaves = bytes(range(64))
    assert gpu.merkle_tree(leaves) == R.digest(R.BLAKE3, leaves)
