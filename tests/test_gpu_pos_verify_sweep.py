"""GPU: the stored-file client checks under many mutations per launch.  lcpc_verify_column_values and
lcpc_verify_leaf_paths answer with one flag per column: the flags must be the exact 0/1 vector the
oracle gives column by column (of_verify_column_value, oracle_ffi.verify_path), with a different
mutation in each of a chosen subset of the columns and honest columns between them -- at 1, 63, 64, 65
and 257 columns, the ends of the kernels' 64-lane groups.  pos.client_verify_evaluations_grouped gets
one honest audit per leaf chunk count, copied once per mutation into a single call that spans several
staging groups and mixes files (so roots): every copy's outcome is the single check's on that copy
alone, and names what the mutation was built for (tests/verify_mut.py: RAW and ALL_BLIND column
changes against the left vector, path levels, result entries)."""
import ctypes as C

import numpy as np
import pytest

import verify_mut as V

pytestmark = pytest.mark.gpu

FT63 = 0
NAMES = {0: "Ft63", 1: "Ft127", 2: "Ft191", 3: "Ft255", 4: "Ft253_192"}
COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    return N


def targets(n: int):
    """the columns of a call that take a mutation: the ends of the 64-lane groups, the first and the
    last column, and every third one; the rest stay honest"""
    return sorted(({0, 1, 62, 63, 64, 65, 127, 128, n - 2, n - 1} | set(range(2, n, 3))) & set(range(n)))


def rounds(mutations, n: int):
    """the mutations dealt onto the target columns of as many calls as it takes: [(column, mutation)]"""
    t = targets(n)
    return [list(zip(t, mutations[i:i + len(t)])) for i in range(0, len(mutations), len(t))]


def u8p(N, a):
    return a.ctypes.data_as(N.u8p)


# ---------------------------------------------------------------- lcpc_verify_column_values
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("fid", V.FIELD_IDS, ids=[NAMES[f] for f in V.FIELD_IDS])
def test_column_values_flag_by_flag(gpu, oracle, native, fid, n):
    """RAW at every row place and the claimed value off by 2^(32 w) for every word w, one mutation per
    target column: ok[] is of_verify_column_value's vector, and its zeros are the mutated columns"""
    nl, p = oracle.limbs(fid), oracle.modulus(fid)
    n_rows = V.rows_for_chunks(fid, 3)
    cols = oracle.ChaCha(seed_u64=300 + fid).field_random(fid, n * n_rows).reshape(n, n_rows * nl)
    t = oracle.ChaCha(seed_u64=301 + fid).field_random(fid, n_rows)
    n_values = n + 3
    idx = np.ascontiguousarray(np.random.default_rng(n).permutation(n_values)[:n].astype(np.uint64))
    values = oracle.ChaCha(seed_u64=302 + fid).field_random(fid, n_values).reshape(n_values, nl)
    for k in range(n):
        values[int(idx[k])] = oracle.collapse(fid, cols[k], t, n_rows, 1)
    mutations = [("row", r) for r in V.row_places(fid, n_rows)] + [("word", w) for w in range(V.field_words(fid))] \
        + [("stored word", w) for w in range(V.field_words(fid))]
    lib = oracle.lib()
    for deal in rounds(mutations, n):
        c, v = cols.copy(), values.copy()
        for k, (what, at) in deal:
            if what == "row":
                c[k] = V.add_delta(fid, c[k], V.blind([], at, 1, n_rows, p), p)
            elif what == "word":
                v[int(idx[k])] = V.shift_value(fid, v[int(idx[k])], at, p)
            else:   # the claim's stored words differ from the sum's in word `at` alone (and by carry)
                v[int(idx[k])] = V.shift_stored(fid, v[int(idx[k])], at, p)
        want = [int(lib.of_verify_column_value(fid, oracle.p64(np.ascontiguousarray(c[k])), oracle.p64(t), n_rows,
                                               oracle.p64(np.ascontiguousarray(v[int(idx[k])])))) for k in range(n)]
        assert [k for k in range(n) if not want[k]] == [k for k, _ in deal]
        ok = np.full(n, 7, np.uint8)
        c, v = np.ascontiguousarray(c.reshape(-1)), np.ascontiguousarray(v.reshape(-1))
        gpu.lcpc2d._raise(native.load().lcpc_verify_column_values(fid, gpu.lcpc2d._p64(c), n, n_rows, gpu.lcpc2d._p64(t),
                                                                  gpu.lcpc2d._p64(v), n_values, gpu.lcpc2d._p64(idx),
                                                                  u8p(native, ok)))
        assert ok.tolist() == want, deal


# ---------------------------------------------------------------- lcpc_verify_leaf_paths
def _tree(oracle, n_leaves: int, seed: int):
    """(leaves, all hashes, root) of random leaf digests under the oracle's merkle_tree"""
    leaves = np.random.default_rng(seed).integers(0, 256, 32 * n_leaves, dtype=np.uint8)
    parents = np.zeros(32 * (n_leaves - 1), np.uint8)
    oracle.lib().of_merkle_tree(leaves.ctypes.data_as(oracle.u8p), n_leaves, parents.ctypes.data_as(oracle.u8p))
    hashes = leaves.tobytes() + parents.tobytes()
    return hashes, hashes[-32:]


def _path(hashes: bytes, n_leaves: int, i: int) -> bytes:
    out, off, width = [], 0, n_leaves
    while width > 1:
        sib = off + (i ^ 1)
        out.append(hashes[32 * sib:32 * sib + 32])
        off += width
        width >>= 1
        i >>= 1
    return b"".join(out)


def _leaf_paths(gpu, native, leaves: bytes, paths: bytes, n: int, path_len: int, idx, root: bytes):
    lv = np.frombuffer(leaves, np.uint8).copy()
    pa = np.frombuffer(paths or b"\0", np.uint8).copy()   # exactly n * path_len digests (one byte when none)
    ix = np.ascontiguousarray(np.array(idx, dtype=np.uint64))
    rt = (C.c_uint8 * 32).from_buffer_copy(root)
    ok = np.full(n, 7, np.uint8)
    gpu.lcpc2d._raise(native.load().lcpc_verify_leaf_paths(u8p(native, lv), u8p(native, pa), n, path_len,
                                                           gpu.lcpc2d._p64(ix), C.cast(rt, native.u8p), u8p(native, ok)))
    return ok.tolist()


@pytest.mark.parametrize("n", COUNTS)
def test_leaf_paths_flag_by_flag(gpu, oracle, native, n):
    """a flipped leaf byte, a flipped path byte at every level and every bit of the index, one per target
    column: ok[] is oracle_ffi.verify_path's vector; its zeros are the mutated columns"""
    n_leaves, path_len = 512, 9
    hashes, root = _tree(oracle, n_leaves, 40 + n)
    where = sorted(np.random.default_rng(n).permutation(n_leaves)[:n].tolist())
    if n > 1:
        where[0], where[-1] = 0, n_leaves - 1
    mutations = [("leaf", 0)] + [("path", i) for i in range(path_len)] + [("index", i) for i in range(path_len)]
    for deal in rounds(mutations, n):
        leaves = [hashes[32 * i:32 * i + 32] for i in where]
        paths = [_path(hashes, n_leaves, i) for i in where]
        idx = list(where)
        for k, (what, i) in deal:
            if what == "leaf":
                leaves[k] = V.flip(leaves[k], 31, k)
            elif what == "path":
                paths[k] = V.flip(paths[k], 32 * i + V.PATH_BYTES[i % 3], k + i)
            else:
                idx[k] ^= 1 << i
        want = [int(oracle.verify_path(leaves[k], idx[k], paths[k], root)) for k in range(n)]
        assert [k for k in range(n) if not want[k]] == [k for k, _ in deal]
        assert _leaf_paths(gpu, native, b"".join(leaves), b"".join(paths), n, path_len, idx, root) == want, deal


@pytest.mark.parametrize("n", [1, 3])
def test_leaf_paths_of_a_one_leaf_tree(gpu, oracle, native, n):
    """path_len = 0: no path digest is read, ok[k] is leaf == root"""
    root = bytes(range(32))
    leaves = [root, V.flip(root, 31, 7), root][:n]
    if n == 1:
        assert _leaf_paths(gpu, native, V.flip(root, 0, 0), b"", 1, 0, [0], root) == [0]
    assert _leaf_paths(gpu, native, b"".join(leaves), b"", n, 0, [0] * n, root) == [int(x == root) for x in leaves]
    assert all(oracle.verify_path(x, 0, b"", root) == (x == root) for x in leaves)


# ---------------------------------------------------------------- client_verify_evaluations_grouped
ROWS = (5, 125, 253, 637)   # 1, 2, 3 and 6 leaf chunks of 8-byte elements


def _honest_audit(gpu, pos, rows, pre, enc, n_open, seed):
    code = gpu.LigeroEncoding.new_from_dims(FT63, pre, enc)
    comm = gpu.LcCommit.commit(gpu.field_random(FT63, rows * pre, 2000 + seed), code)
    point = gpu.field_random(FT63, 1, 2100 + seed)
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(point, rows, pre)
    result = pos.verifiable_polynomial_evaluation(comm, left)
    cols = sorted(np.random.default_rng(seed).permutation(enc)[:n_open].tolist())
    return (comm.get_root(), 7 * rows * pre, pre, enc, point, cols, result, comm.open_columns(cols)), left


def _with_column(gpu, audit, k, col=None, path=None):
    columns = list(audit[7])
    columns[k] = gpu.LcColumn(columns[k].col if col is None else col, list(columns[k].path) if path is None else path)
    return audit[:7] + (columns,)


def _result_verdict(oracle, audit, res):
    """what the check says to a changed result vector, the columns and paths being honest: the vector is
    decoded, its first pre coefficients are encoded again and compared at the opened indices with
    <left, column>, which for honest columns is the honest result's entry"""
    pre, enc, cols, honest = audit[2], audit[3], audit[5], np.asarray(audit[6]).reshape(-1)
    coeffs = oracle.ifft_oi(FT63, np.ascontiguousarray(res, dtype=np.uint64).reshape(-1))
    row = np.zeros(enc, np.uint64)
    row[:pre] = coeffs[:pre]
    again = oracle.fft_io(FT63, row)
    return "values" if any(again[j] != honest[j] for j in cols) else "ok"


def _mutations(gpu, oracle, audit, left):
    """[(label, audit, what it must report: "paths", "values" or "ok")] of one honest audit"""
    p = oracle.modulus(FT63)
    rows, cols, columns = left.shape[0], audit[5], audit[7]
    u = [V.canon(FT63, left)]
    ks = sorted({0, 1, 62, 63, 64, 65, len(cols) - 1} & set(range(len(cols))))
    out = []
    for cls in (V.RAW, V.ALL_BLIND):   # any change of a column changes its leaf: the paths fail first;
        for r in V.row_places(FT63, rows):   # ALL_BLIND keeps <left, column>, so nothing but the leaf sees it
            delta = V.blind(u if cls == V.ALL_BLIND else [], r, 1, rows, p)
            assert (V.dot(u[0], delta, p) == 0) == (cls == V.ALL_BLIND)
            for k in ks:
                out.append((f"{cls} col {k} row {r}", _with_column(gpu, audit, k, col=V.add_delta(FT63, columns[k].col, delta, p)),
                            "paths"))
    for k in ks:
        for level in range(len(columns[k].path)):
            for b in V.PATH_BYTES:
                path = list(columns[k].path)
                path[level] = V.flip(path[level], b, k + level + b)
                out.append((f"path col {k} level {level} byte {b}", _with_column(gpu, audit, k, path=path), "paths"))
    closed = [j for j in range(audit[3]) if j not in cols]
    for j in list(cols) + closed[:1]:
        res = np.array(audit[6], dtype=np.uint64, copy=True)
        res.reshape(-1)[j] = V.other_element(FT63, res.reshape(-1)[j:j + 1], p)[0]
        want = _result_verdict(oracle, audit, res)
        # an opened entry no longer matches its column; a closed one moves the decoded prefix, and with it
        # the entries encoded again at the opened indices: the result vector is bound as a whole
        assert want == "values"
        out.append((f"result entry {j}" + (" (closed)" if j in closed else ""), audit[:6] + (res, audit[7]), want))
    return out


def _names(x):
    if isinstance(x, np.ndarray):
        return "ok"
    text = str(x).lower()
    return "paths" if "path" in text else "values" if "value" in text else text


@pytest.mark.parametrize("pre,enc,n_open", [(8, 16, 12), (16, 64, 63)], ids=["8x16", "16x64"])
def test_grouped_audits_copy_by_copy(gpu, oracle, pos, monkeypatch, pre, enc, n_open):
    honest = [_honest_audit(gpu, pos, rows, pre, enc, n_open, 10 * enc + i) for i, rows in enumerate(ROWS)]
    assert [int(V.n_chunks(FT63, r)) for r in ROWS] == [1, 2, 3, 6] and len({a[0] for a, _ in honest}) == len(ROWS)
    assert _result_verdict(oracle, honest[0][0], honest[0][0][6]) == "ok"
    per_file = [_mutations(gpu, oracle, a, left) for a, left in honest]
    # the files take turns, an honest copy after every third mutation: neighbours differ in root
    jobs, turn = [], 0
    while any(per_file):
        for f, muts in enumerate(per_file):
            if muts:
                jobs.append(muts.pop(0))
                turn += 1
                if turn % 3 == 0:
                    jobs.append((f"honest copy of file {f}", honest[f][0], "ok"))
    audits = [a for _, a, _ in jobs]
    # the staging seam at four of the largest jobs' column bytes: the call spans many groups
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(4 * 8 * ROWS[-1] * n_open))
    _, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    assert launches >= 8
    got = pos.client_verify_evaluations_grouped(audits)
    assert len(got) == len(jobs)
    values = {}
    for (label, audit, want), g in zip(jobs, got):
        try:
            one = pos.client_verify_evaluation(*audit)
        except gpu.VerifierError as e:
            one = e
        assert _names(g) == _names(one) == want, (label, g, one)
        if want == "ok":
            assert g.shape == one.shape and g.dtype == one.dtype and np.array_equal(g, one), label
            assert np.array_equal(values.setdefault(audit[0], g), g), label   # every copy of a file: one value
        else:
            assert isinstance(g, gpu.VerifierError) and g.kind == one.kind == "ColumnEval", label
    assert len(values) == len(ROWS)
    print(f"{len(jobs)} jobs, {launches} launches")
