"""GPU: batched evaluation proofs (lcpc_prove_batch / lcpc_verify_batch) in lockstep with the
Python reference tests/batch_ref.py: p_random, every p_eval_j, the opened columns (hence the column
indices), the paths and a challenge drawn afterwards from both transcripts; m = 1 against
lcpc_prove; the other digests; the evaluations against Python integers; the caller-transcript
forms; a device-rebuilt commitment; the byte layout; and forged proofs, each with its error kind.

Forged p_eval vectors: every p_eval is absorbed before the column challenge, so changing one
redraws the columns.  A forgery that keeps the old columns shows them at the wrong indices and
fails the first per-column check (ColumnDegree); the forgeries below therefore reopen the columns,
honestly, where the changed proof's own challenge falls (batch_ref.reopen) -- a forger's best
follow-up -- and must be caught by the evaluation check itself (ColumnEval)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import batch_ref as B

pytestmark = pytest.mark.gpu

FT63, FT127, FT191, FT255, FT253_192 = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def _case(kind, fid, lg):
    """product and oracle encodings of one shape, coefficients and both commitments"""
    import lcpc_proof_of_storage_amd as L
    import oracle_ffi as O
    if kind == "ligero":
        enc = L.LigeroEncoding.new(fid, 1 << lg)
        n = 1 << lg
    elif kind == "ligero_ml":
        enc = L.LigeroEncoding.new_ml(fid, lg)
        n = 1 << lg
    elif kind == "rs":  # plain R-S, 3 rows
        enc = L.RsEncoding.new(fid, 1 << lg, 2 << lg, 20, 2)
        n = 3 << lg
    else:  # SDIG code 3
        enc = L.SdigEncoding.new(fid, 1 << lg, 0, 3)
        n = 1 << lg
    if kind == "sdig":
        o_enc = O.Encoding.sdig(fid, enc.n_per_row, seed=0, code_id=3)
    else:
        o_enc = O.Encoding.ligero(fid, enc.n_per_row, enc.n_cols, enc.get_n_col_opens(), enc.get_n_degree_tests())
    assert (o_enc.n_cols, o_enc.n_col_opens, o_enc.n_degree_tests) == \
        (enc.n_cols, enc.get_n_col_opens(), enc.get_n_degree_tests())
    coeffs = O.random_coeffs(fid, n, 77 + fid + lg)
    comm = L.LcCommit.commit(coeffs, enc)
    o_comm = O.Commit(o_enc, coeffs)
    assert comm.get_root() == o_comm.root()
    return dict(fid=fid, enc=enc, o_enc=o_enc, coeffs=coeffs, comm=comm, o_comm=o_comm, root=o_comm.root(),
                nr=o_comm.n_rows, npr=o_comm.n_per_row, nc=o_comm.n_cols, nl=O.limbs(fid))


@functools.lru_cache(maxsize=None)
def _points(fid, npr, nr, m, seed=5):
    import oracle_ffi as O
    xs = O.ChaCha(seed_u64=seed + 31 * m + fid).field_random(fid, m).reshape(m, -1)
    pts = [O.eval_tensors(fid, xs[j], npr, nr) for j in range(m)]
    return xs, [p[0] for p in pts], [p[1] for p in pts]


def _g_tr(L, c):
    tr = L.Transcript(b"test transcript")
    tr.append_message(b"polycommit", c["root"])
    tr.append_message(b"ncols", c["enc"].get_n_col_opens().to_bytes(8, "big"))
    return tr


def _o_tr(c):
    import oracle_ffi as O
    return O.standard_transcript(c["enc"].get_n_col_opens(), c["root"])


def _as_ref(pf, nl) -> "B.BatchProof":
    cols = pf.columns
    return B.BatchProof(pf.field, pf.n_cols, [v.reshape(-1) for v in pf.p_eval_vec],
                        [v.reshape(-1) for v in pf.p_random_vec], [],
                        [c.col.reshape(-1) for c in cols], [b"".join(c.path) for c in cols])


def _as_product(L, ref: "B.BatchProof", nl):
    cols = [L.LcColumn(col.reshape(-1, nl), [p[i:i + 32] for i in range(0, len(p), 32)])
            for col, p in zip(ref.cols, ref.paths)]
    return L.LcBatchEvalProof.from_parts(ref.fid, ref.n_cols, ref.p_evals, ref.p_random, cols)


def _assert_same(pf, ref: "B.BatchProof"):
    got = _as_ref(pf, None)
    assert len(got.p_evals) == len(ref.p_evals) and len(got.p_random) == len(ref.p_random)
    for j, (a, b) in enumerate(zip(got.p_evals, ref.p_evals)):
        assert np.array_equal(a, b), f"p_eval {j}"
    for i, (a, b) in enumerate(zip(got.p_random, ref.p_random)):
        assert np.array_equal(a, b), f"p_random {i}"
    assert len(got.cols) == len(ref.cols)
    for k, (a, b) in enumerate(zip(got.cols, ref.cols)):  # equal columns <=> equal column indices
        assert np.array_equal(a, b), f"column {k} (index {ref.col_idx[k]})"
    assert got.paths == ref.paths


def _lockstep(gpu, c, m):
    xs, inners, outers = _points(c["fid"], c["npr"], c["nr"], m)
    tg, to = _g_tr(gpu, c), _o_tr(c)
    pf = c["comm"].prove_batch(outers, c["enc"], tg)
    ref = B.prove_batch(c["o_comm"], c["o_enc"], outers, to)
    assert pf.n_evals == m
    _assert_same(pf, ref)
    assert tg.challenge_bytes(b"after", 32) == to.challenge_bytes(b"after", 32)
    vg, vo = _g_tr(gpu, c), _o_tr(c)
    evs = pf.verify(c["root"], outers, inners, c["enc"], vg)
    kind, want = B.verify_batch(c["root"], outers, inners, ref, c["o_enc"], vo)
    assert kind == 0 and len(evs) == m
    for j in range(m):
        assert np.array_equal(evs[j], want[j]), f"evaluation {j}"
    assert vg.challenge_bytes(b"after", 32) == vo.challenge_bytes(b"after", 32)
    return pf, ref


@pytest.mark.parametrize("m", [1, 2, 5, 9])
@pytest.mark.parametrize("fid", [FT63, FT127, FT255])
def test_ligero_lockstep(gpu, fid, m):
    _lockstep(gpu, _case("ligero", fid, 10), m)


@pytest.mark.parametrize("kind,fid,lg,m", [("ligero", FT191, 8, 3), ("ligero", FT253_192, 8, 3), ("rs", FT63, 5, 4),
                                           ("sdig", FT127, 12, 3), ("ligero_ml", FT127, 10, 3)])
def test_other_encodings_lockstep(gpu, kind, fid, lg, m):
    _lockstep(gpu, _case(kind, fid, lg), m)


@pytest.mark.parametrize("kind,fid,lg", [("ligero", FT63, 10), ("ligero", FT127, 10), ("ligero", FT253_192, 8),
                                         ("sdig", FT127, 12)])
def test_one_evaluation_is_lcpc_prove(gpu, kind, fid, lg):
    c = _case(kind, fid, lg)
    xs, inners, outers = _points(fid, c["npr"], c["nr"], 1)
    ta, tb = _g_tr(gpu, c), _g_tr(gpu, c)
    batch = c["comm"].prove_batch(outers, c["enc"], ta)
    single = c["comm"].prove(outers[0], c["enc"], tb)
    assert ta.challenge_bytes(b"after", 32) == tb.challenge_bytes(b"after", 32)
    assert np.array_equal(batch.p_eval_vec[0], single.p_eval)
    # the batch layout with one evaluation = the single proof's bytes plus the count of p_eval vectors
    sb, bb = single.to_bincode(), batch.to_bytes()
    assert bb == sb[:8] + (1).to_bytes(8, "little") + sb[8:]
    va, vb = _g_tr(gpu, c), _g_tr(gpu, c)
    ev = batch.verify(c["root"], outers, inners, c["enc"], va)
    assert np.array_equal(ev[0], single.verify(c["root"], outers[0], inners[0], c["enc"], vb))
    assert va.challenge_bytes(b"after", 32) == vb.challenge_bytes(b"after", 32)


@pytest.mark.parametrize("digest", [1, 3], ids=["sha256", "keccak256"])
def test_other_digests_differ_in_paths_only(gpu, digest):
    c = _case("ligero", FT127, 10)
    xs, inners, outers = _points(FT127, c["npr"], c["nr"], 3)
    base = c["comm"].prove_batch(outers, c["enc"], _g_tr(gpu, c))
    enc = gpu.LigeroEncoding.new(FT127, 1 << 10).set_digest(digest)
    comm = gpu.LcCommit.commit(c["coeffs"], enc)
    assert comm.get_root() != c["root"]
    pf = comm.prove_batch(outers, enc, _g_tr(gpu, c))  # seeded alike: the same challenges
    a, b = _as_ref(pf, None), _as_ref(base, None)
    assert all(np.array_equal(x, y) for x, y in zip(a.p_evals + a.p_random + a.cols, b.p_evals + b.p_random + b.cols))
    assert a.paths != b.paths
    evs = pf.verify(comm.get_root(), outers, inners, enc, _g_tr(gpu, c))
    want = base.verify(c["root"], outers, inners, c["enc"], _g_tr(gpu, c))
    assert all(np.array_equal(x, y) for x, y in zip(evs, want))
    with pytest.raises(gpu.VerifierError) as e:  # the BLAKE3 root under the other digest's paths
        pf.verify(c["root"], outers, inners, enc, _g_tr(gpu, c))
    assert e.value.kind == "ColumnPath"
    with pytest.raises(gpu.LcpcError) as e:  # a commitment and an encoding of different digests
        c["comm"].prove_batch(outers, enc, _g_tr(gpu, c))
    assert e.value.code == 30


@pytest.mark.parametrize("fid", [FT63, FT127])
def test_evaluations_are_the_polynomials(gpu, oracle, fid):
    c = _case("ligero", fid, 10)
    xs, inners, outers = _points(fid, c["npr"], c["nr"], 4)
    pf = c["comm"].prove_batch(outers, c["enc"], _g_tr(gpu, c))
    evs = pf.verify(c["root"], outers, inners, c["enc"], _g_tr(gpu, c))
    p = oracle.modulus(fid)
    cs = oracle.from_mont(fid, c["coeffs"])
    for j in range(4):
        x = oracle.from_mont(fid, xs[j])[0]
        want = 0
        for v in reversed(cs):
            want = (want * x + v) % p
        assert oracle.from_mont(fid, evs[j])[0] == want, f"point {j}"


class _Forwarding:
    """a caller-owned transcript: merlin's two methods onto a library transcript"""

    def __init__(self, tr):
        self.tr = tr

    def append_message(self, label, msg):
        self.tr.append_message(label, msg)

    def challenge_bytes(self, label, n):
        return self.tr.challenge_bytes(label, n)


def test_ops_forms_give_the_same_bytes(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    lib = N.load()
    c = _case("ligero", FT127, 10)
    m = 3
    xs, inners, outers = _points(FT127, c["npr"], c["nr"], m)
    want = c["comm"].prove_batch(outers, c["enc"], _g_tr(gpu, c))
    # the mirror with a caller transcript object
    fw = _Forwarding(_g_tr(gpu, c))
    via_obj = c["comm"].prove_batch(outers, c["enc"], fw)
    assert via_obj.to_bytes() == want.to_bytes()
    # lcpc_prove_batch_ops / lcpc_verify_batch_ops with the caller's ops table
    o = np.ascontiguousarray(np.stack([np.asarray(t).reshape(-1) for t in outers]))
    i = np.ascontiguousarray(np.stack([np.asarray(t).reshape(-1) for t in inners]))
    p64 = gpu.lcpc2d._p64
    ct = gpu.CallerTranscript(_Forwarding(_g_tr(gpu, c)))
    h = C.c_void_p()
    assert lib.lcpc_prove_batch_ops(c["comm"]._h, p64(o.reshape(-1)), m, c["nr"], c["enc"]._h, C.byref(ct._ops),
                                    C.byref(h)) == 0
    via_ops = gpu.LcBatchEvalProof(h.value)
    assert via_ops.to_bytes() == want.to_bytes()
    rp = (C.c_uint8 * 32).from_buffer_copy(c["root"])
    out = np.zeros((m, c["nl"]), np.uint64)
    cv = gpu.CallerTranscript(_Forwarding(_g_tr(gpu, c)))
    assert lib.lcpc_verify_batch_ops(rp, p64(o.reshape(-1)), m, c["nr"], p64(i.reshape(-1)), c["npr"], via_ops._h,
                                     c["enc"]._h, C.byref(cv._ops), p64(out.reshape(-1))) == 0
    evs = want.verify(c["root"], outers, inners, c["enc"], _g_tr(gpu, c))
    assert all(np.array_equal(out[j], evs[j]) for j in range(m))
    assert lib.lcpc_prove_batch_ops(c["comm"]._h, p64(o.reshape(-1)), m, c["nr"], c["enc"]._h, None, C.byref(h)) == 30


def test_rebuilt_commitment_and_serde(gpu):
    c = _case("ligero", FT127, 10)
    xs, inners, outers = _points(FT127, c["npr"], c["nr"], 5)
    want = c["comm"].prove_batch(outers, c["enc"], _g_tr(gpu, c))
    rebuilt = gpu.LcCommit.from_bincode(FT127, c["comm"].to_bincode())
    again = rebuilt.prove_batch(outers, c["enc"], _g_tr(gpu, c))
    data = want.to_bytes()
    assert again.to_bytes() == data
    back = gpu.LcBatchEvalProof.from_bytes(FT127, data)
    assert back.to_bytes() == data and back.n_evals == 5
    evs = back.verify(c["root"], outers, inners, c["enc"], _g_tr(gpu, c))
    ref = want.verify(c["root"], outers, inners, c["enc"], _g_tr(gpu, c))
    assert all(np.array_equal(a, b) for a, b in zip(evs, ref))
    assert data == B.to_bytes(_as_ref(want, None))
    for bad in (data[:-3], data + b"\0"):
        with pytest.raises(gpu.LcpcError):
            gpu.LcBatchEvalProof.from_bytes(FT127, bad)


# ---------------------------------------------------------------- forgeries
@pytest.fixture(scope="module")
def forge(gpu):
    c = _case("ligero", FT127, 10)
    m = 5
    xs, inners, outers = _points(FT127, c["npr"], c["nr"], m)
    pf = c["comm"].prove_batch(outers, c["enc"], _g_tr(gpu, c))
    return dict(c=c, m=m, inners=inners, outers=outers, ref=_as_ref(pf, None))


def _verdict(gpu, f, ref, outers=None, inners=None):
    c = f["c"]
    pf = _as_product(gpu, ref, c["nl"])
    try:
        pf.verify(c["root"], f["outers"] if outers is None else outers, f["inners"] if inners is None else inners,
                  c["enc"], _g_tr(gpu, c))
    except gpu.LcpcError as e:
        return e
    return None


def _copy(ref, **kw):
    d = dict(ref.__dict__)
    d.update(kw)
    return B.BatchProof(**d)


def test_untouched_rebuild_verifies(gpu, forge):
    assert _verdict(gpu, forge, forge["ref"]) is None
    assert _verdict(gpu, forge, B.reopen(forge["c"]["o_comm"], forge["c"]["o_enc"], forge["ref"], _o_tr(forge["c"]))) is None


@pytest.mark.parametrize("which", ["first", "last"])
def test_forged_p_eval_word(gpu, forge, which):
    c, ref = forge["c"], forge["ref"]
    j = 0 if which == "first" else forge["m"] - 1
    evals = [v.copy() for v in ref.p_evals]
    evals[j][3] ^= np.uint64(1)
    bad = _copy(ref, p_evals=evals)
    e = _verdict(gpu, forge, B.reopen(c["o_comm"], c["o_enc"], bad, _o_tr(c)))
    assert e is not None and e.kind == "ColumnEval"
    assert f"evaluation {j}" in str(e)  # lcpc_last_error names the first failing j
    # the old columns kept: they sit at the wrong indices, and the first per-column check says so
    e = _verdict(gpu, forge, bad)
    assert e is not None and e.kind == "ColumnDegree"


def test_swapped_p_eval_vectors(gpu, forge):
    c, ref = forge["c"], forge["ref"]
    bad = _copy(ref, p_evals=[ref.p_evals[1], ref.p_evals[0]] + ref.p_evals[2:])
    e = _verdict(gpu, forge, B.reopen(c["o_comm"], c["o_enc"], bad, _o_tr(c)))
    assert e is not None and e.kind == "ColumnEval" and "evaluation 0" in str(e)


def test_forged_p_random_word(gpu, forge):
    c, ref = forge["c"], forge["ref"]
    pr = [v.copy() for v in ref.p_random]
    pr[0][1] ^= np.uint64(4)
    bad = _copy(ref, p_random=pr)
    for attempt in (bad, B.reopen(c["o_comm"], c["o_enc"], bad, _o_tr(c))):
        e = _verdict(gpu, forge, attempt)
        assert e is not None and e.kind == "ColumnDegree"


def test_forged_column_word_and_path_byte(gpu, forge):
    ref = forge["ref"]
    cols = [v.copy() for v in ref.cols]
    cols[2][0] ^= np.uint64(1)
    e = _verdict(gpu, forge, _copy(ref, cols=cols))
    assert e is not None and e.kind == "ColumnDegree"  # by precedence: the evaluation and the path fail too
    paths = list(ref.paths)
    paths[1] = paths[1][:40] + bytes([paths[1][40] ^ 1]) + paths[1][41:]
    e = _verdict(gpu, forge, _copy(ref, paths=paths))
    assert e is not None and e.kind == "ColumnPath"


def test_argument_errors(gpu, forge):
    c, ref, m = forge["c"], forge["ref"], forge["m"]
    outers, inners = forge["outers"], forge["inners"]
    e = _verdict(gpu, forge, ref, outers=[outers[1], outers[0]] + outers[2:])
    assert e is not None and e.kind == "ColumnEval" and "evaluation 0" in str(e)
    e = _verdict(gpu, forge, ref, outers=outers[:-1], inners=inners[:-1])  # proof count != call count
    assert e is not None and e.kind == "OuterTensor"
    e = _verdict(gpu, forge, ref, inners=[np.concatenate([v, v[:c["nl"]]]) for v in inners])
    assert e is not None and e.kind == "InnerTensor"
    e = _verdict(gpu, forge, ref, outers=[v[:-c["nl"]] for v in outers])
    assert e is not None and e.kind == "OuterTensor"
    # m = 0, at the C boundary and through the mirror
    from lcpc_proof_of_storage_amd import _native as N
    lib = N.load()
    z = np.zeros(4, np.uint64)
    p64 = gpu.lcpc2d._p64
    h = C.c_void_p()
    tr = _g_tr(gpu, c)
    assert lib.lcpc_prove_batch(c["comm"]._h, p64(z), 0, c["nr"], c["enc"]._h, tr._h, C.byref(h)) == 30
    assert lib.lcpc_prove_batch(c["comm"]._h, p64(z), gpu.BATCH_MAX_TENSORS + 1, c["nr"], c["enc"]._h, tr._h,
                                C.byref(h)) == 30
    pf = _as_product(gpu, ref, c["nl"])
    rp = (C.c_uint8 * 32).from_buffer_copy(c["root"])
    assert lib.lcpc_verify_batch(rp, p64(z), 0, c["nr"], p64(z), c["npr"], pf._h, c["enc"]._h, tr._h, None) == 30
    with pytest.raises(gpu.LcpcError) as ei:
        c["comm"].prove_batch([], c["enc"], _g_tr(gpu, c))
    assert ei.value.code == 30
    with pytest.raises(gpu.ProverError) as ei:
        c["comm"].prove_batch([v[:-c["nl"]] for v in outers], c["enc"], _g_tr(gpu, c))
    assert ei.value.kind == "OuterTensor"


# ---------------------------------------------------------------- full size
@pytest.mark.slow
@pytest.mark.timeout(600)
def test_full_size_ft127_2p24_sixteen_points(gpu, oracle):
    """The headline shape (Ft127, 2^24 coefficients, 512 x 32768 -> 65536), m = 16, in full lockstep
    with batch_ref: the oracle's sixteen row combinations run on up to 16 CPU threads."""
    oracle.lib().of_set_threads(min(16, len(os.sched_getaffinity(0))))
    fid, n, m = FT127, 1 << 24, 16
    coeffs = oracle.random_coeffs(fid, n)
    enc = gpu.LigeroEncoding.new(fid, n)
    comm = gpu.LcCommit.commit(coeffs, enc)
    o_enc = oracle.Encoding.ligero_new(fid, n)
    o_comm = oracle.Commit(o_enc, coeffs)
    assert comm.get_root() == o_comm.root()
    c = dict(fid=fid, enc=enc, o_enc=o_enc, coeffs=coeffs, comm=comm, o_comm=o_comm, root=o_comm.root(),
             nr=o_comm.n_rows, npr=o_comm.n_per_row, nc=o_comm.n_cols, nl=2)
    assert (c["nr"], c["npr"], c["nc"]) == (512, 32768, 65536)
    _lockstep(gpu, c, m)
