"""GPU: the threading contract of include/lcpc_mi.h -- "handles may be used from several threads".

Every other GPU parity test is serial.  Here one child process (tests/_threads_child.py) runs up to
16 host threads on the library at once, through the raw C entry points with the GIL released, and
writes what it got to a file; this module computes the CPU oracle's answers serially and compares
bytes and limbs, exactly.  A block of the exact-size cache recycled into another thread's stream
too early, a staging slot shared by two threads, a four-step intermediate handed to two encodes:
each would show as a wrong row, root, proof or evaluation below.

  A  the reference's rayon encode: 16 threads, lcpc_encode on disjoint rows of one encoding, at the
     smallest length of every transform path (LDS row, four-step for two fields, the stored
     files' Ft63 dims) and one Brakedown encoding;
  B  16 threads, each commit / prove / verify of its own polynomial three times over on ONE
     encoding (handles freed in between, so blocks of one size go round); then 8 threads on two
     encodings of different fields and block sizes;
  C  one commitment handle: 8 provers with different tensors and 8 column openers at once; then
     16 verifiers of one proof handle;
  D  the server's request mix: a different stateless entry point per thread, twice round;
  E  lcpc_last_error is per thread: a failing call's message reaches only its own thread;
  F  B's first half again on a second generation of threads.

The child runs under the default stream mode and under LCPC_STREAM_MODE=serial (every thread's
calls on one stream).  For A, B and D under the default mode the recorded windows of the native
calls must overlap between threads -- otherwise the run was serial and proved nothing; the share
of calls that overlapped another thread's is printed.  A deadlock ends in a killed child whose
stderr names its threads (faulthandler), not in a stalled suite."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("LCPC_NO_MFMA", "LCPC_STREAM_MODE", "LCPC_PRIORITY_STREAMS", "LCPC_HOST_WAIT", "LCPC_KECCAK",
         "LCPC_ROW1_PREFETCH", "LCPC_ROW1_GLDS", "LCPC_SHARD_BULK_STREAMS")
SETTINGS = {"default": {}, "serial": {"LCPC_STREAM_MODE": "serial"}}
_expected = {}  # the oracle's answers, computed once and shared by both settings; never modified


@pytest.fixture(scope="module")
def TC(gpu):
    import _threads_child
    return _threads_child


@pytest.fixture(scope="module", params=list(SETTINGS))
def run(request, gpu, tmp_path_factory):
    """(setting, {key: array}) of one child process"""
    path = str(tmp_path_factory.mktemp("threads") / f"{request.param}.npz")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(SETTINGS[request.param])
    r = subprocess.run([sys.executable, os.path.join(HERE, "_threads_child.py"), path], env=env,
                       capture_output=True, text=True, timeout=150)
    if r.returncode != 0:
        print(r.stderr[-6000:])
    assert r.returncode == 0, (request.param, r.stderr[-3000:])
    with np.load(path) as z:
        data = {k.replace("__", "/"): z[k] for k in z.files}
    os.remove(path)
    return request.param, data


def overlap_share(calls):
    """the share of native calls whose window overlaps a call of ANOTHER thread"""
    th, t0, t1 = calls[:, 0], calls[:, 1], calls[:, 2]
    hit = (t0[:, None] < t1[None, :]) & (t0[None, :] < t1[:, None]) & (th[:, None] != th[None, :])
    return float(hit.any(axis=1).mean())


def check_overlap(run, name):
    setting, data = run
    share = overlap_share(data[f"calls/{name}"])
    print(f"scenario {name} [{setting}]: {len(data[f'calls/{name}'])} native calls, "
          f"{100 * share:.0f}% overlapped a call of another thread")
    if setting == "default":
        assert share > 0, f"scenario {name}: no two threads' calls overlapped: the run was serial"


def expected(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def _frozen(a):
    a = np.array(a)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- A
def _a_expected(TC, oracle):
    res = {}
    shapes = [(name, field, n_cols // 2, n_cols, 100 + i) for i, (name, field, n_cols) in enumerate(TC.A_SHAPES)]
    for name, field, npr, n_cols, seed in shapes:
        rows = TC.plan_a_rows(field, npr, n_cols, seed)
        res[name] = _frozen(np.stack([oracle.fft_io(field, r.reshape(-1)).reshape(r.shape) for r in rows]))
    name, field, length, seed = TC.A_SDIG
    import lcpc_proof_of_storage_amd as L
    g_enc = L.SdigEncoding.new(field, length, seed)
    o_enc = oracle.Encoding.sdig(field, g_enc.n_per_row, seed=seed, code_id=3)
    assert o_enc.n_cols == g_enc.n_cols
    rows = TC.plan_a_rows(field, g_enc.n_per_row, g_enc.n_cols, 150)
    res[name] = _frozen(np.stack([o_enc.encode(r.reshape(-1)).reshape(r.shape) for r in rows]))
    return res


def test_a_encode_rows_of_one_encoding_from_16_threads(run, TC, oracle):
    """the reference's commit: rayon workers encode disjoint rows of one encoding
    (lcpc-2d/src/lib.rs:677-682); every row of every shape is the oracle's codeword"""
    want = expected("A", lambda: _a_expected(TC, oracle))
    data = run[1]
    for name, rows in want.items():
        got = data[f"A/{name}"]
        assert got.shape == rows.shape
        bad = [r for r in range(rows.shape[0]) if not np.array_equal(got[r], rows[r])]
        assert not bad, f"{name}: rows {bad} differ from the oracle's codewords (row r ran on thread r mod {TC.T})"
    check_overlap(run, "A")


# ---------------------------------------------------------------- B, F
def _b_expected(TC, oracle, tag, t, shape):
    """the oracle's commit (once) and, per iteration, proof / evaluation / transcript end states"""
    field, npr, n_cols, _ = shape
    coeffs, outer, inner = TC.plan_b_poly(tag, t, shape)
    o_enc = oracle.Encoding.ligero(field, npr, n_cols, TC.B_NCO, TC.B_NDT)
    o = oracle.Commit(o_enc, coeffs.reshape(-1))
    root = o.root()
    its = []
    for it in range(TC.B_ITERS):
        def tr():
            x = oracle.Transcript(b"test transcript")
            x.append_message(b"polycommit", TC.plan_b_prefix(tag, t, it))
            x.append_message(b"ncols", TC.B_NCO.to_bytes(8, "big"))
            return x
        p_tr, v_tr = tr(), tr()
        op = o.prove(o_enc, outer.reshape(-1), p_tr)
        rc, ev = op.verify(root, outer.reshape(-1), inner.reshape(-1), o_enc, v_tr)
        assert rc == 0
        its.append(dict(p_eval=_frozen(op.p_eval), p_random=_frozen(op.p_random), cols=_frozen(op.cols),
                        paths=_frozen(op.paths), ev=_frozen(ev),
                        after=p_tr.challenge_bytes(b"after", 32) + v_tr.challenge_bytes(b"after", 32)))
    return root, its


def _check_proof(data, key, want, where):
    """field by field, as test_gpu_transcript_ops._same_proof"""
    for f in ("p_eval", "p_random", "cols", "paths"):
        assert np.array_equal(data[f"{key}/{f}"], want[f]), f"{where}: {f} differs from the oracle's"


def _check_commitments(run, TC, oracle, name, tag, shapes):
    data = run[1]
    for t, shape in enumerate(shapes):
        root, its = expected(("B", tag, t, shape), lambda: _b_expected(TC, oracle, tag, t, shape))
        for it, want in enumerate(its):
            key, where = f"{name}/{t}/{it}", f"{name}: thread {t}, iteration {it}, field {shape[0]}"
            assert data[f"{key}/root"].tobytes() == root, f"{where}: root differs from the oracle's"
            _check_proof(data, key, want, where)
            assert np.array_equal(data[f"{name}/{t}/evals"][it], want["ev"]), f"{where}: evaluation"
            assert data[f"{key}/after"].tobytes() == want["after"], f"{where}: transcript end state"


def test_b_commit_prove_verify_per_thread_on_one_encoding(run, TC, oracle):
    """16 threads x 3 iterations on the cfg1 shape: root, p_eval, every p_random, every opened
    column and path, the evaluation and both transcripts' end states are the oracle's"""
    _check_commitments(run, TC, oracle, "B", 1, [TC.B_MAIN] * TC.T)
    check_overlap(run, "B")


def test_b_two_encodings_of_different_fields_at_once(run, TC, oracle):
    """8 threads, four on Ft63 2048 -> 4096 and four on Ft127 4096 -> 8192 (four-step): block sizes
    and fields interleave"""
    _check_commitments(run, TC, oracle, "B2", 2, [TC.B_MIXED[t % 2] for t in range(8)])
    check_overlap(run, "B2")


def test_f_second_generation_of_threads(run, TC, oracle):
    """B's first half on fresh threads after the first set has exited (its thread_local pinned
    slots and events destroyed, its released blocks still fenced): the same bytes"""
    _check_commitments(run, TC, oracle, "F", 1, [TC.B_MAIN] * TC.T)
    data = run[1]
    for k in [k for k in data if k.startswith("B/")]:
        assert np.array_equal(data[k], data["F/" + k[2:]]), k


# ---------------------------------------------------------------- C
def _c_expected(TC, oracle):
    field, npr, n_cols, _ = TC.B_MAIN
    o_enc = oracle.Encoding.ligero(field, npr, n_cols, TC.B_NCO, TC.B_NDT)
    coeffs = TC.plan_b_poly(3, 0, TC.B_MAIN)[0]
    o = oracle.Commit(o_enc, coeffs.reshape(-1))
    root = o.root()
    proofs = []
    for k in range(8):
        outer, _ = TC.plan_c(k)
        op = o.prove(o_enc, outer.reshape(-1), oracle.standard_transcript(TC.B_NCO, root))
        proofs.append(dict(p_eval=_frozen(op.p_eval), p_random=_frozen(op.p_random), cols=_frozen(op.cols),
                           paths=_frozen(op.paths)))
        if k == 0:
            rc, ev = op.verify(root, outer.reshape(-1), TC.plan_c(0)[1].reshape(-1), o_enc,
                               oracle.standard_transcript(TC.B_NCO, root))
            assert rc == 0
    comm = o.comm.reshape(o.n_rows, n_cols, -1)
    return dict(root=root, proofs=proofs, ev=_frozen(ev), columns=_frozen(comm[:, TC.C_COLUMNS].transpose(1, 0, 2)))


def test_c_one_commitment_and_one_proof_handle_from_many_threads(run, TC, oracle):
    """8 lcpc_prove and 8 x 4 lcpc_open_column on ONE commitment handle at once: each proof is the
    oracle's, each opened column the oracle's column and the serial call's column and path; then
    16 lcpc_verify of one proof handle: every evaluation the oracle's"""
    want = expected("C", lambda: _c_expected(TC, oracle))
    data = run[1]
    assert data["C/root"].tobytes() == want["root"]
    for k in range(8):
        _check_proof(data, f"C/{k}", want["proofs"][k], f"C: prover {k}")
    assert np.array_equal(data["C/cols"], want["columns"])
    assert np.array_equal(data["C/cols"], data["C/serial_cols"])
    assert np.array_equal(data["C/paths"], data["C/serial_paths"])
    for t in range(TC.T):
        assert np.array_equal(data["C/evals"][t], want["ev"]), f"C: verifier {t}"
    check_overlap((run[0] + " (reported only)", data), "C")


# ---------------------------------------------------------------- D, E
def _d_expected(TC, oracle, job, t, rnd):
    import ctypes as C
    import update_ref as R
    from pyref import FIELD_DECL
    a = TC.plan_d(job, t, rnd)
    if job == "pos_commit":
        return np.frombuffer(oracle.pos_encode_file(a["data"].tobytes(), *TC.D_POS_DIMS)[1][-32:], np.uint8)
    if job == "hash_columns":
        return np.frombuffer(oracle.hash_columns(a["field"], a["m"].reshape(-1), a["n_rows"], a["n_cols"]), np.uint8)
    if job == "merkle_tree":
        leaves, parents = np.ascontiguousarray(a["leaves"]), np.zeros(32 * 1023, np.uint8)
        oracle.lib().of_merkle_tree(leaves.ctypes.data_as(C.POINTER(C.c_uint8)), 1024,
                                    parents.ctypes.data_as(C.POINTER(C.c_uint8)))
        return parents
    if job == "left_multiply":
        from test_gpu_pos_batch_audit import reference
        return reference(a["data"].tobytes(), a["pre"], a["left"].reshape(1, -1))[0]
    if job in TC.D_ERASURE:
        nl = oracle.limbs(a["field"])
        rows = np.zeros((3, a["length"] * nl), np.uint64)
        rows[:, :a["npr"] * nl] = a["msgs"].reshape(3, -1)
        return np.stack([oracle.fft_io(a["field"], r) for r in rows]).reshape(3, a["length"], nl)
    p = FIELD_DECL[a["field"]][0]
    canon = oracle.from_mont(a["field"], a["coeffs"].reshape(-1))
    xv = oracle.from_mont(a["field"], a["x"].reshape(-1))[0]
    return oracle.to_mont(a["field"], [R.horner(canon, xv, a["degree"], p)])


def test_d_request_mix_of_stateless_entry_points(run, TC, oracle):
    """16 threads, a different stateless entry point per thread and round, each against the
    reference its own test uses"""
    data = run[1]
    for t in range(TC.T):
        for rnd in range(TC.D_ROUNDS):
            job = TC.d_job(t, rnd)
            want = expected(("D", t, rnd), lambda: _frozen(_d_expected(TC, oracle, job, t, rnd)))
            got = data[f"D/{t}/{rnd}"]
            assert np.array_equal(got.reshape(-1), want.reshape(-1)), f"D: thread {t}, round {rnd}: {job}"
    check_overlap(run, "D")


def test_e_last_error_is_per_thread(run, TC):
    """while the others work, one thread's lcpc_encode with a wrong length fails with
    LCPC_ERR_INVALID_ARG (before any launch) and reads its own message, still there after its later
    successful calls; a thread that only succeeded reads the empty message it started with"""
    data = run[1]
    msg = bytes(data["E/failed_msg"].astype(np.uint8))
    assert int(data["E/failed_rc"]) == TC.INVALID_ARG
    assert b"SDIG encode: slice length" in msg, msg
    assert bytes(data["E/failed_msg_end"].astype(np.uint8)) == msg
    assert data["E/quiet_before"].size == 0 and data["E/quiet_after"].size == 0
