"""GPU: every word of a proof decides the verifier's verdict.  LcEvalProof.verify and
LcBatchEvalProof.verify on proofs the GPU made, rebuilt with one mutation each (tests/verify_mut.py):
the outcome must be the oracle's on the same words -- accepted with the evaluation equal word for
word, or the exact VerifierError kind.  The mutations separate the three per-column checks: RAW dies
at the degree test, DEGREE_BLIND passes it and dies at the evaluation (in a batch: at the evaluation
it aims at, which the message names), ALL_BLIND passes both and only the column's leaf hash sees it;
RAW_TOP moves the first check's sum in its top stored word alone (a comparison short of one word).
They sit where the kernels can go wrong: the opened columns around a 64-lane group (k_path_checks,
k_path_checks_digest: one column per lane) and around flag 63/64 of k_column_checks' 64-thread blocks
over (column, tensor) pairs; the first and last row of every 1-KiB leaf chunk, at 1, 2 (the fused
two-chunk kernel), 3, 9 (serial merge) and 17 chunks (merge in groups of 8), for Ft63 with even
(column-major kernel) and odd row counts (strided kernel), for Ft191 the element across the chunk
edge (the word kernel); every 32-bit word of an element; every path level; every root byte.

test_verify_mut.py shows on the CPU that each class gets its verdict from the oracle and that no
case is left out; here each case counts its mutations against the same table.

A one-column tree is not swept: RsEncoding admits no n_cols = 1 (no redundancy); the one-row
commitment at (8, 16) is."""
import collections
import time

import numpy as np
import pytest

import digest_ref as R
import verify_mut as V

pytestmark = pytest.mark.gpu

NAMES = {0: "Ft63", 1: "Ft127", 2: "Ft191", 3: "Ft255", 4: "Ft253_192"}
DIGEST_FIELDS = (1, 2, 4)


def _transcript(L, root: bytes, n_open: int):
    tr = L.Transcript(b"test transcript")
    tr.append_message(b"polycommit", root)
    tr.append_message(b"ncols", int(n_open).to_bytes(8, "big"))
    return tr


def _encoding(L, case, digest=R.BLAKE3):
    s = case["shape"]
    enc = L.RsEncoding.new(case["fid"], s.n_per_row, s.n_cols, s.n_open, case["ndt"])
    return enc.set_digest(digest) if digest != R.BLAKE3 else enc


def _gpu_context(L, case, batch: bool, digest=R.BLAKE3):
    """commit and prove on the GPU; the proof as plain words in a verify_mut context.  The transcript
    is seeded with the BLAKE3 root whatever the digest, so every digest draws the same challenges."""
    s = case["shape"]
    enc = _encoding(L, case, digest)
    comm = L.LcCommit.commit(case["coeffs"], enc)
    root = comm.get_root()
    assert (root == case["root"]) == (digest == R.BLAKE3)
    tr = _transcript(L, case["root"], s.n_open)
    pf = comm.prove_batch(case["outers"], enc, tr) if batch else comm.prove(case["outers"][0], enc, tr)
    ctx = V.context(V.from_product(pf), root, case["outers"], case["inners"], case["o_enc"],
                    lambda: V.O.standard_transcript(s.n_open, case["root"]))
    return enc, ctx


def _outcome(L, enc, case, bp, root, batch: bool, outers=None, inners=None):
    """(status code, evaluations, message) of the GPU verifier on these words"""
    outers = case["outers"] if outers is None else outers
    inners = case["inners"] if inners is None else inners
    pf = V.product_proof(L, bp, batch)
    tr = _transcript(L, case["root"], case["shape"].n_open)
    try:
        if batch:
            return 0, pf.verify(root, outers, inners, enc, tr), ""
        return 0, [pf.verify(root, outers[0], inners[0], enc, tr)], ""
    except L.VerifierError as e:
        return e.code, None, str(e)


def _same_evaluations(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(w).reshape(-1))


def _honest(L, enc, case, ctx, batch, oracle_ctx=None):
    """the untouched proof: accepted, the evaluations the oracle's; under another point: the oracle's
    rejection (the tensors are not in the transcript, so the evaluation check is what fails).  A
    one-row proof has the outer tensor [1] at every point and is accepted, with the other inner
    tensor's value."""
    o = oracle_ctx or ctx
    kind, want = V.oracle_verdict(o, o.proof)
    assert kind == V.OK
    code, evs, _ = _outcome(L, enc, case, ctx.proof, ctx.root, batch)
    assert code == 0
    _same_evaluations(evs, want)
    s = case["shape"]
    inners2, outers2 = V.points(case["fid"], s.n_per_row, s.n_rows, case["m"], seed=99)
    kind, want2 = V.oracle_verdict(o, o.proof, outers=outers2, inners=inners2)
    assert kind == (V.COLUMN_EVAL if s.n_rows > 1 else V.OK)
    code, evs2, msg = _outcome(L, enc, case, ctx.proof, ctx.root, batch, outers2, inners2)
    assert code == kind, msg
    if kind == V.OK:
        _same_evaluations(evs2, want2)
        assert not np.array_equal(np.asarray(evs2[0]).reshape(-1), np.asarray(evs[0]).reshape(-1))
    return 2


def _sweep(L, enc, case, ctx, batch: bool):
    """every mutation of verify_mut.sweep through the GPU verifier; returns the verify calls made"""
    seen = collections.Counter()
    for mut in V.sweep(ctx, case["shape"]):
        want, evs = V.verdict(ctx, mut)
        if mut.expect is not None:
            assert want == mut.expect, (mut.cls, mut.where, V.KIND.get(want, want))
        code, got, msg = _outcome(L, enc, case, mut.proof, mut.root, batch)
        assert code == want, (mut.cls, mut.where, V.KIND.get(code, code), V.KIND.get(want, want), msg)
        if want == V.OK:
            _same_evaluations(got, evs)
        if batch and want == V.COLUMN_EVAL and mut.cls in (V.RAW, V.DEGREE_BLIND):
            assert f"(evaluation {mut.aim or 0})" in msg, (mut.where, msg)
        seen[mut.cls] += 1
    want = V.sweep_counts(case["fid"], case["shape"], case["ndt"], case["m"])
    assert {c: seen[c] for c in want} == want and seen[V.EXCHANGE] >= 2
    return sum(seen.values())


SINGLE = [(fid, chunks, ndt) for fid in V.FIELD_IDS for chunks in (0,) + V.CHUNK_CLASSES[fid] for ndt in V.NDTS]


@pytest.mark.parametrize("fid,chunks,ndt", SINGLE,
                         ids=[f"{NAMES[f]}-{'row1' if c == 0 else f'chunks{c}'}-ndt{n}" for f, c, n in SINGLE])
def test_single_proof(gpu, fid, chunks, ndt):
    t0, calls = time.perf_counter(), 0
    for shape in ([V.ONE_ROW] if chunks == 0 else V.single_shapes(fid, chunks)):
        assert chunks == 0 or V.n_chunks(fid, shape.n_rows) == chunks
        case = V.oracle_case(fid, shape, ndt)
        enc, ctx = _gpu_context(gpu, case, batch=False)
        calls += _honest(gpu, enc, case, ctx, False) + _sweep(gpu, enc, case, ctx, False)
    print(f"verify calls {calls}, {time.perf_counter() - t0:.2f} s")


BATCH = [(fid, m, ndt) for fid in V.BATCH_FIELDS for m in V.BATCH_MS for ndt in V.BATCH_NDTS]


@pytest.mark.parametrize("fid,m,ndt", BATCH, ids=[f"{NAMES[f]}-m{m}-ndt{n}" for f, m, n in BATCH])
def test_batch_proof(gpu, fid, m, ndt):
    """the same sweep against batch_ref.verify_batch; DEGREE_BLIND aimed at each evaluation in turn"""
    t0 = time.perf_counter()
    case = V.oracle_case(fid, V.batch_shape(fid), ndt, m)
    enc, ctx = _gpu_context(gpu, case, batch=True)
    calls = _honest(gpu, enc, case, ctx, True) + _sweep(gpu, enc, case, ctx, True)
    print(f"verify calls {calls}, {time.perf_counter() - t0:.2f} s")


def _climb(d: int, leaf: bytes, col: int, path) -> bytes:
    """verify_column_path's climb (lcpc-2d/src/lib.rs:985-1012) with digest d"""
    h = leaf
    for sib in path:
        h = R.digest(d, h + sib if col % 2 == 0 else sib + h)
        col >>= 1
    return h


@pytest.mark.parametrize("d", [R.SHA256, R.SHA3_256, R.KECCAK256], ids=["sha256", "sha3_256", "keccak256"])
@pytest.mark.parametrize("fid", DIGEST_FIELDS, ids=[NAMES[f] for f in DIGEST_FIELDS])
def test_other_digests(gpu, fid, d):
    """The oracle hashes with BLAKE3 only.  The digest's proof holds the BLAKE3 proof's vectors and
    columns (the transcripts are seeded alike) and other paths, so each mutation is made on both: the
    digest's run must give what the oracle gives the BLAKE3 one.  For ALL_BLIND, path and root
    mutations that is ColumnPath by construction; digest_ref confirms on the CPU that the changed
    column's leaf differs from the committed one and that the committed one climbs to the root."""
    t0 = time.perf_counter()
    shape = V.single_shapes(fid, 2)[0]
    case = V.oracle_case(fid, shape, 1)
    ctx_b = V.oracle_context(case)
    enc, ctx_d = _gpu_context(gpu, case, batch=False, digest=d)
    a, b = ctx_b.proof, ctx_d.proof
    assert all(np.array_equal(x, y) for x, y in zip(a.p_evals + a.p_random + a.cols, b.p_evals + b.p_random + b.cols))
    assert a.paths != b.paths and ctx_b.idx == ctx_d.idx
    calls = _honest(gpu, enc, case, ctx_d, False, oracle_ctx=ctx_b)
    seen, blind = collections.Counter(), []
    for mut_b, mut in zip(V.sweep(ctx_b, shape), V.sweep(ctx_d, shape)):
        assert (mut_b.cls, mut_b.where) == (mut.cls, mut.where)
        assert all(np.array_equal(x, y) for x, y in zip(mut_b.proof.cols, mut.proof.cols))
        want, _ = V.verdict(ctx_b, mut_b)
        if mut.cls in (V.ALL_BLIND, V.PATH, V.ROOT):
            assert want == mut.expect == V.COLUMN_PATH
        code, got, msg = _outcome(gpu, enc, case, mut.proof, mut.root, False)
        assert code == want, (mut.cls, mut.where, V.KIND.get(code, code), V.KIND.get(want, want), msg)
        assert want != V.OK or got is not None
        if mut.cls == V.ALL_BLIND:
            blind.append((mut.k, mut.proof.cols[mut.k]))
        seen[mut.cls] += 1
    want = V.sweep_counts(fid, shape, 1)
    assert {c: seen[c] for c in want} == want and len(blind) == want[V.ALL_BLIND] > 0
    leaves = R.digest_many(d, [bytes(32) + R.column_bytes(fid, col) for _, col in blind])
    honest = {k: R.leaf(d, fid, ctx_d.proof.cols[k]) for k in {k for k, _ in blind}}
    for k, lf in honest.items():
        path = ctx_d.proof.paths[k]
        assert _climb(d, lf, ctx_d.idx[k], [path[i:i + 32] for i in range(0, len(path), 32)]) == ctx_d.root
    assert all(lf != honest[k] for (k, _), lf in zip(blind, leaves))
    print(f"verify calls {calls + sum(seen.values())}, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- free functions
@pytest.mark.parametrize("d,fid", [(R.BLAKE3, f) for f in V.FIELD_IDS] + [(d, f) for d, f in
                                                                         zip((R.SHA256, R.SHA3_256, R.KECCAK256), DIGEST_FIELDS)],
                         ids=lambda v: str(v))
def test_verify_column_path_needs_every_index_bit(gpu, oracle, d, fid):
    """verify_column_path at col_num with one bit flipped is False for every level, True at col_num:
    against the oracle's climb (BLAKE3) resp. digest_ref's."""
    shape = V.single_shapes(fid, 3)[0]
    case = V.oracle_case(fid, shape, 1)
    comm = gpu.LcCommit.commit(case["coeffs"], _encoding(gpu, case, d))
    root = comm.get_root()
    path_len = shape.n_cols.bit_length() - 1
    for col_num in (0, 1, 0b1010101, shape.n_cols - 1):
        c = comm.open_column(col_num)
        assert len(c.path) == path_len
        if d == R.BLAKE3:
            leaf = oracle.hash_columns(fid, c.col.reshape(-1), shape.n_rows, 1)
            climb = lambda i: oracle.verify_path(leaf, i, b"".join(c.path), root)   # noqa: E731
        else:
            leaf = R.leaf(d, fid, c.col)
            climb = lambda i: _climb(d, leaf, i, c.path) == root                      # noqa: E731
        assert climb(col_num) and gpu.verify_column_path(fid, c, col_num, root, digest=d)
        for i in range(path_len):
            other = col_num ^ (1 << i)
            assert not climb(other)
            assert not gpu.verify_column_path(fid, c, other, root, digest=d), (col_num, i)


@pytest.mark.parametrize("fid", V.FIELD_IDS, ids=[NAMES[f] for f in V.FIELD_IDS])
def test_verify_column_value_needs_every_word(gpu, oracle, fid):
    """a claimed value off by 2^(32 w) is refused for every word w of the element, as a canonical value
    and as stored words (which the kernel compares: a comparison over all words but one accepts the
    latter), as by of_verify_column_value; the dot product itself is accepted"""
    nl, p = oracle.limbs(fid), oracle.modulus(fid)
    n_rows = V.rows_for_chunks(fid, 3)
    col = oracle.ChaCha(seed_u64=61 + fid).field_random(fid, n_rows)
    t = oracle.ChaCha(seed_u64=62 + fid).field_random(fid, n_rows)
    value = oracle.collapse(fid, col, t, n_rows, 1)
    column = gpu.LcColumn(col.reshape(-1, nl), [])

    def both(claim):
        want = bool(oracle.lib().of_verify_column_value(fid, oracle.p64(col), oracle.p64(t), n_rows,
                                                        oracle.p64(np.ascontiguousarray(claim))))
        assert gpu.verify_column_value(fid, column, t, claim) == want
        return want

    assert both(value)
    for w in range(V.field_words(fid)):
        assert not both(V.shift_value(fid, value, w, p)), w
        # the same in the stored words: the claim and the sum then differ in word w alone (and by carry)
        assert not both(V.shift_stored(fid, value, w, p)), w
