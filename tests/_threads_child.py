"""Child process of test_gpu_threads.py: one process, up to 16 host threads on the library at once.

The header promises that handles may be used from several threads (include/lcpc_mi.h); every call
leases a stream from a per-device pool, takes its device blocks from one exact-size cache and
stages through thread_local pinned slots.  Here the scenarios of test_gpu_threads.py run with all
ctypes arguments prepared before a threading.Barrier, the threads then call the raw lib.lcpc_*
functions (a C.CDLL: the GIL is released for the whole native call), and what the handles hold is
read after join (scenario B, which frees its handles between iterations, copies them out into
arrays made before the barrier).  This process does not load the oracle: it writes every output, and the
perf_counter_ns window of every native call, to the .npz named on argv[1]; the parent computes
the oracle's answers serially and compares.  The inputs are functions of seeds (the plan_*
functions below), which the parent calls too.

A stall ends with faulthandler's dump of every thread a little before the parent's timeout; an
exception in any thread is recorded and makes the exit status 1."""
import ctypes as C
import faulthandler
import os
import sys
import threading
import time
import traceback

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcpc_proof_of_storage_amd as L  # noqa: E402
from lcpc_proof_of_storage_amd import _native as N  # noqa: E402

T = 16                     # threads at once, at the most (bench.py's loop runs as many)
STALL_DUMP_S = 135         # (the parent's timeout is 150 s)
INVALID_ARG = 30
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)

# ---- scenario A: (name, field, n_cols) -- rate 1/2 rows, 64 per shape
A_ROWS = 64
A_SHAPES = [("ft127_lds", 1, 1 << 12),      # the whole row in LDS
            ("ft127_4step", 1, 1 << 13),    # the smallest four-step length: intermediate from the block pool
            ("ft255_4step", 3, 1 << 13),
            ("ft63_pos", 0, 1 << 15)]       # the stored files' dims
A_SDIG = ("sdig_ft127", 1, 1 << 12, 0)      # SdigEncoding.new(1, 1 << 12, 0): one lcpc_encode per codeword

# ---- scenario B: (field, n_per_row, n_cols, coefficients); 128 column openings, 2 degree tests
B_NCO, B_NDT, B_ITERS = 128, 2, 3
B_MAIN = (1, 2048, 4096, 1 << 16)           # the cfg1 shape, 32 rows
B_MIXED = [(0, 2048, 4096, 1 << 16),        # Ft63 at the same dims ...
           (1, 4096, 8192, 1 << 16)]        # ... and Ft127 four-step, 16 rows: four threads each
C_COLUMNS = [0, 1, 77, 2047, 2048, 3001, 4094, 4095]
D_POS_DIMS = (64, 128)
D_JOBS = ("pos_commit", "hash_columns", "merkle_tree", "left_multiply", "erasure_small", "erasure_big", "eval_poly")
D_ROUNDS = 2
D_ERASURE = {"erasure_small": (3, 16, 32), "erasure_big": (1, 512, 1024)}  # field, n_per_row, len; 3 rows


def p64(a):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(N.u64p)


def p8(a):
    assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(N.u8p)


# ---------------------------------------------------------------- the inputs (parent and child)
def plan_a_rows(field, n_per_row, n_cols, seed):
    """(A_ROWS, n_cols, limbs): random coefficients in the first n_per_row places, zero above"""
    nl = L.limbs(field)
    rows = np.zeros((A_ROWS, n_cols, nl), np.uint64)
    rows[:, :n_per_row] = L.field_random(field, A_ROWS * n_per_row, seed).reshape(A_ROWS, n_per_row, nl)
    return rows


def plan_b_poly(tag, t, shape):
    """thread t's polynomial, outer and inner tensors in run `tag` (a seed of its own)"""
    field, n_per_row, _, length = shape
    seed = 1000 * tag + 10 * t
    n_rows = -(-length // n_per_row)
    return (L.field_random(field, length, seed + 1), L.field_random(field, n_rows, seed + 2),
            L.field_random(field, n_per_row, seed + 3))


def plan_b_prefix(tag, t, it):
    """what stands in the transcript where tests put the root (which no thread knows before the
    barrier): 32 bytes naming the run, thread and iteration"""
    return bytes([tag, t, it]) + bytes(29)


def plan_c(k):
    """prover k's outer tensor and inner tensor for the shared commitment"""
    field, n_per_row, _, length = B_MAIN
    return L.field_random(field, length // n_per_row, 7000 + k), L.field_random(field, n_per_row, 7100 + k)


def plan_d(job, t, rnd):
    """the inputs of thread t's round-rnd call of stateless entry point `job`"""
    seed = 9000 + 100 * t + rnd
    rng = np.random.default_rng(seed)
    if job == "pos_commit":
        return dict(data=rng.integers(0, 256, 100_000 + 7 * t + 3 * rnd + 1, dtype=np.uint8))
    if job == "hash_columns":
        field = t % 2
        return dict(field=field, n_rows=37, n_cols=256, m=L.field_random(field, 37 * 256, seed))
    if job == "merkle_tree":
        return dict(leaves=rng.integers(0, 256, 32 * 1024, dtype=np.uint8))
    if job == "left_multiply":  # pre 64, 17 rows (the last one partial)
        return dict(data=rng.integers(0, 256, 7 * 64 * 17 - 5 - t, dtype=np.uint8), pre=64,
                    left=L.field_random(0, 17, seed))
    if job in D_ERASURE:
        field, npr, length = D_ERASURE[job]
        erased = np.sort(rng.permutation(length)[:length - npr]).astype(np.uint64)
        return dict(field=field, npr=npr, length=length, erased=erased,
                    msgs=L.field_random(field, 3 * npr, seed).reshape(3, npr, L.limbs(field)))
    if job == "eval_poly":
        field = t % 2
        return dict(field=field, n=1000 + t, degree=37 + rnd, coeffs=L.field_random(field, 1000 + t, seed),
                    x=L.field_random(field, 1, seed + 50))
    raise KeyError(job)


def d_job(t, rnd):
    return D_JOBS[(t + 3 * rnd) % len(D_JOBS)]


# ---------------------------------------------------------------- running threads
class Threads:
    """n threads behind one barrier; each records the window of every native call and its exception"""

    def __init__(self, out, name):
        self.out, self.name = out, name
        self.errors = []

    def run(self, bodies):
        n = len(bodies)
        assert n <= T
        barrier = threading.Barrier(n)
        windows = [[] for _ in range(n)]

        def main(i):
            def call(fn, *a):
                t0 = time.perf_counter_ns()
                rc = fn(*a)
                windows[i].append((i, t0, time.perf_counter_ns()))
                return rc
            try:
                barrier.wait(timeout=60)
                bodies[i](call)
            except BaseException:  # noqa: BLE001 -- recorded; the child exits non-zero
                self.errors.append(f"{self.name} thread {i}:\n{traceback.format_exc()}")
                barrier.abort()

        ths = [threading.Thread(target=main, args=(i,), name=f"{self.name}-{i}") for i in range(n)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        w = [x for ws in windows for x in ws]
        key = f"calls/{self.name}"
        prev = self.out.get(key)
        cur = np.array(w, np.int64).reshape(-1, 3)
        self.out[key] = cur if prev is None else np.concatenate([prev, cur])
        return self.errors


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: status {rc}: {N.last_error()}")


# ---------------------------------------------------------------- A: the rayon encode
def scenario_a(lib, out, errors):
    encs, rows = [], []
    for i, (name, field, n_cols) in enumerate(A_SHAPES):
        encs.append(L.RsEncoding.new(field, n_cols // 2, n_cols, 16, 1))
        rows.append(plan_a_rows(field, n_cols // 2, n_cols, 100 + i))
    name, field, length, seed = A_SDIG
    sdig = L.SdigEncoding.new(field, length, seed)
    encs.append(sdig)
    rows.append(plan_a_rows(field, sdig.n_per_row, sdig.n_cols, 150))
    # thread t: rows r = t mod T of every shape, the shapes interleaved (block sizes then mix)
    jobs = [[] for _ in range(T)]
    for r in range(A_ROWS):
        for e, m in zip(encs, rows):
            row_bytes = m[r].nbytes
            jobs[r % T].append((e._h, C.cast(m.ctypes.data + r * row_bytes, N.u64p), m.shape[1]))

    def body(t):
        def run(call):
            for h, ptr, n in jobs[t]:
                ok(call(lib.lcpc_encode, h, ptr, n), "lcpc_encode")
        return run

    errors += Threads(out, "A").run([body(t) for t in range(T)])
    for (name, *_), m in zip(A_SHAPES + [A_SDIG], rows):
        out[f"A/{name}"] = m


# ---------------------------------------------------------------- B / F: independent commitments
def _transcript(prefix, nco):
    tr = L.Transcript(b"test transcript")
    tr.append_message(b"polycommit", prefix)
    tr.append_message(b"ncols", nco.to_bytes(8, "big"))
    return tr


def _save_proof(out, key, h):
    """the fields _same_proof compares, flat"""
    pf = L.LcEvalProof(h)  # (frees the handle when it goes)
    out[f"{key}/p_eval"] = pf.p_eval.reshape(-1)
    pr = pf.p_random_vec
    out[f"{key}/p_random"] = np.concatenate([v.reshape(-1) for v in pr]) if pr else np.zeros(0, np.uint64)
    cols = pf.columns
    out[f"{key}/cols"] = np.concatenate([c.col.reshape(-1) for c in cols])
    out[f"{key}/paths"] = np.frombuffer(b"".join(b"".join(c.path) for c in cols), np.uint8)


def commitments(lib, out, errors, name, tag, shapes_of_threads):
    """every thread: B_ITERS x (lcpc_commit_new from host memory, lcpc_prove with a library
    transcript, lcpc_verify), the commitment freed after its prove and the proof (copied out into
    arrays made before the barrier) after its verify, so that device blocks and page-locked
    blocks of the same exact sizes go round between the threads"""
    n = len(shapes_of_threads)
    encs = {s: L.RsEncoding.new(s[0], s[1], s[2], B_NCO, B_NDT) for s in set(shapes_of_threads)}
    st = []
    for t, shape in enumerate(shapes_of_threads):
        coeffs, outer, inner = plan_b_poly(tag, t, shape)
        nl, n_rows, pl = L.limbs(shape[0]), -(-shape[3] // shape[1]), L.log2(shape[2])
        st.append(dict(p_eval=np.zeros((B_ITERS, shape[1], nl), np.uint64),
                       p_random=np.zeros((B_ITERS, B_NDT, shape[1], nl), np.uint64),
                       cols=np.zeros((B_ITERS, B_NCO, n_rows, nl), np.uint64),
                       paths=np.zeros((B_ITERS, B_NCO, 32 * pl), np.uint8),
                       enc=encs[shape]._h, coeffs=coeffs, outer=outer, inner=inner, n=coeffs.shape[0],
                       roots=[(C.c_uint8 * 32)() for _ in range(B_ITERS)],
                       p_tr=[_transcript(plan_b_prefix(tag, t, it), B_NCO) for it in range(B_ITERS)],
                       v_tr=[_transcript(plan_b_prefix(tag, t, it), B_NCO) for it in range(B_ITERS)],
                       proofs=[C.c_void_p() for _ in range(B_ITERS)],
                       evals=np.zeros((B_ITERS, L.limbs(shape[0])), np.uint64)))

    def body(t):
        s = st[t]

        def run(call):
            for it in range(B_ITERS):
                h = C.c_void_p()
                ok(call(lib.lcpc_commit_new, s["enc"], p64(s["coeffs"]), s["n"], C.byref(h)), "lcpc_commit_new")
                try:
                    ok(lib.lcpc_commit_get_root(h, C.cast(s["roots"][it], N.u8p)), "lcpc_commit_get_root")
                    ok(call(lib.lcpc_prove, h, p64(s["outer"]), s["outer"].shape[0], s["enc"], s["p_tr"][it]._h,
                            C.byref(s["proofs"][it])), "lcpc_prove")
                finally:
                    lib.lcpc_commit_free(h)
                pf = s["proofs"][it]
                try:
                    ok(call(lib.lcpc_verify, C.cast(s["roots"][it], N.u8p), p64(s["outer"]), s["outer"].shape[0],
                            p64(s["inner"]), s["inner"].shape[0], pf, s["enc"], s["v_tr"][it]._h,
                            p64(s["evals"][it])), "lcpc_verify")
                    ok(lib.lcpc_proof_copy_p_eval(pf, p64(s["p_eval"][it])), "lcpc_proof_copy_p_eval")
                    for i in range(B_NDT):
                        ok(lib.lcpc_proof_copy_p_random(pf, i, p64(s["p_random"][it, i])), "lcpc_proof_copy_p_random")
                    for k in range(B_NCO):
                        ok(lib.lcpc_proof_copy_column(pf, k, p64(s["cols"][it, k]), p8(s["paths"][it, k])),
                           "lcpc_proof_copy_column")
                finally:
                    lib.lcpc_proof_free(pf)
        return run

    errors += Threads(out, name).run([body(t) for t in range(n)])
    for t, s in enumerate(st):
        out[f"{name}/{t}/evals"] = s["evals"]
        for it in range(B_ITERS):
            key = f"{name}/{t}/{it}"
            out[f"{key}/root"] = np.frombuffer(bytes(s["roots"][it]), np.uint8)
            for f in ("p_eval", "p_random", "cols", "paths"):
                out[f"{key}/{f}"] = s[f][it].reshape(-1)
            # the transcripts' end states too
            out[f"{key}/after"] = np.frombuffer(s["p_tr"][it].challenge_bytes(b"after", 32)
                                                + s["v_tr"][it].challenge_bytes(b"after", 32), np.uint8)


# ---------------------------------------------------------------- C: one handle, many callers
def scenario_c(lib, out, errors):
    shape = B_MAIN
    field, n_per_row, n_cols, length = shape
    nl = L.limbs(field)
    enc = L.RsEncoding.new(field, n_per_row, n_cols, B_NCO, B_NDT)
    coeffs = plan_b_poly(3, 0, shape)[0]
    g = L.LcCommit.commit(coeffs, enc)
    root = g.get_root()
    n_rows, pl = g.get_n_rows(), L.log2(n_cols)
    out["C/root"] = np.frombuffer(root, np.uint8)
    tensors = [plan_c(k) for k in range(8)]
    p_tr = [_transcript(root, B_NCO) for _ in range(8)]
    proofs = [C.c_void_p() for _ in range(8)]
    cols = np.zeros((8, n_rows, nl), np.uint64)
    paths = np.zeros((8, 32 * pl), np.uint8)

    def prover(k):
        def run(call):
            ok(call(lib.lcpc_prove, g._h, p64(tensors[k][0]), n_rows, enc._h, p_tr[k]._h, C.byref(proofs[k])),
               "lcpc_prove")
        return run

    def opener(k):
        def run(call):
            for _ in range(4):  # (the same answer every time)
                ok(call(lib.lcpc_open_column, g._h, C_COLUMNS[k], p64(cols[k]), p8(paths[k])), "lcpc_open_column")
        return run

    errors += Threads(out, "C").run([prover(k) for k in range(8)] + [opener(k) for k in range(8)])
    out["C/cols"], out["C/paths"] = cols, paths
    serial = [g.open_column(c) for c in C_COLUMNS]
    out["C/serial_cols"] = np.stack([c.col for c in serial])
    out["C/serial_paths"] = np.stack([np.frombuffer(b"".join(c.path), np.uint8) for c in serial])
    if errors:
        return
    # 16 verifiers of ONE proof handle (prover 0's), each with its own transcript
    v_tr = [_transcript(root, B_NCO) for _ in range(T)]
    evals = np.zeros((T, nl), np.uint64)
    rp = (C.c_uint8 * 32).from_buffer_copy(root)
    outer, inner = tensors[0]

    def verifier(t):
        def run(call):
            ok(call(lib.lcpc_verify, C.cast(rp, N.u8p), p64(outer), n_rows, p64(inner), n_per_row, proofs[0], enc._h,
                    v_tr[t]._h, p64(evals[t])), "lcpc_verify")
        return run

    errors += Threads(out, "C").run([verifier(t) for t in range(T)])
    out["C/evals"] = evals
    for k in range(8):
        if proofs[k].value:
            _save_proof(out, f"C/{k}", proofs[k].value)


# ---------------------------------------------------------------- D + E: the server's request mix
def scenario_d(lib, out, errors):
    pos_enc = L.LigeroEncoding.new_from_dims(0, *D_POS_DIMS)
    sdig = L.SdigEncoding.new(A_SDIG[1], A_SDIG[2], A_SDIG[3])
    bad_row = np.zeros((sdig.n_cols + 1, L.limbs(A_SDIG[1])), np.uint64)
    prepared = {}
    for t in range(T):
        for rnd in range(D_ROUNDS):
            job = d_job(t, rnd)
            a = plan_d(job, t, rnd)
            if job == "pos_commit":
                a["h"] = C.c_void_p()
            elif job == "hash_columns":
                a["out"] = np.zeros(32 * a["n_cols"], np.uint8)
            elif job == "merkle_tree":
                a["out"] = np.zeros(32 * 1023, np.uint8)
            elif job == "left_multiply":
                a["out"] = np.zeros(a["pre"], np.uint64)
            elif job in D_ERASURE:
                # the codewords: this library's own encode, serially; the parent compares the decoded
                # rows with the oracle's codewords, so a wrong survivor shows there too
                nl = L.limbs(a["field"])
                rows = np.zeros((3, a["length"], nl), np.uint64)
                rows[:, :a["npr"]] = a["msgs"]
                e = L.RsEncoding.new(a["field"], a["npr"], a["length"], 1, 1)
                ok(lib.lcpc_encode_rows(e._h, p64(rows.reshape(-1)), 3, a["length"]), "lcpc_encode_rows")
                rows[:, a["erased"].astype(np.int64)] = ONES
                a["rows"] = rows
            elif job == "eval_poly":
                a["out"] = np.zeros(L.limbs(a["field"]), np.uint64)
            prepared[t, rnd] = (job, a)
    msgs = {}

    def run_job(call, job, a):
        if job == "pos_commit":
            ok(call(lib.lcpc_pos_commit_bytes, pos_enc._h, p8(a["data"]), a["data"].size, C.byref(a["h"])),
               "lcpc_pos_commit_bytes")
        elif job == "hash_columns":
            ok(call(lib.lcpc_hash_columns, a["field"], p64(a["m"]), a["n_rows"], a["n_cols"], p8(a["out"])),
               "lcpc_hash_columns")
        elif job == "merkle_tree":
            ok(call(lib.lcpc_merkle_tree, p8(a["leaves"]), 1024, p8(a["out"])), "lcpc_merkle_tree")
        elif job == "left_multiply":
            ok(call(lib.lcpc_pos_left_multiply_bytes, p8(a["data"]), a["data"].size, a["pre"], p64(a["left"]), 17,
                    p64(a["out"])), "lcpc_pos_left_multiply_bytes")
        elif job in D_ERASURE:
            ok(call(lib.lcpc_rs_erasure_decode_rows, a["field"], p64(a["rows"]), 3, a["length"], a["npr"],
                    p64(a["erased"]), a["erased"].size), "lcpc_rs_erasure_decode_rows")
        else:
            ok(call(lib.lcpc_eval_poly, a["field"], p64(a["coeffs"]), a["n"], p64(a["x"]), a["degree"],
                    p64(a["out"])), "lcpc_eval_poly")

    def body(t):
        def run(call):
            before = lib.lcpc_last_error() or b""
            if t == T - 1:
                # E: a call that must fail before any launch; its message is this thread's own
                rc = lib.lcpc_encode(sdig._h, p64(bad_row), bad_row.shape[0])
                msgs["failed_rc"] = rc
                msgs["failed_msg"] = lib.lcpc_last_error() or b""
            for rnd in range(D_ROUNDS):
                run_job(call, *prepared[t, rnd])
            if t == T - 2:
                msgs["quiet_before"], msgs["quiet_after"] = before, lib.lcpc_last_error() or b""
            if t == T - 1:
                msgs["failed_msg_end"] = lib.lcpc_last_error() or b""
        return run

    errors += Threads(out, "D").run([body(t) for t in range(T)])
    for k, v in msgs.items():
        out[f"E/{k}"] = np.array(v if isinstance(v, int) else list(v), np.int64)
    for (t, rnd), (job, a) in prepared.items():
        key = f"D/{t}/{rnd}"
        if job == "pos_commit":
            if a["h"].value:
                c = L.LcCommit(a["h"].value, 0)
                out[key] = np.frombuffer(c.get_root(), np.uint8)
        elif job in D_ERASURE:
            out[key] = a["rows"]
        else:
            out[key] = a["out"]


def main():
    path = sys.argv[1]
    faulthandler.dump_traceback_later(STALL_DUMP_S, exit=True)
    assert L.device_count() > 0, "no HIP device"
    L.set_device(0)
    lib = N.load()
    out, errors = {}, []
    scenario_a(lib, out, errors)
    commitments(lib, out, errors, "B", 1, [B_MAIN] * T)
    commitments(lib, out, errors, "B2", 2, [B_MIXED[t % 2] for t in range(8)])
    scenario_c(lib, out, errors)
    scenario_d(lib, out, errors)
    # F: B's first half again on fresh threads: the first generation's thread_local pinned slots
    # and events are gone, the blocks it released still carry its fences
    commitments(lib, out, errors, "F", 1, [B_MAIN] * T)
    np.savez(path, **{k.replace("/", "__"): v for k, v in out.items()})
    faulthandler.cancel_dump_traceback_later()
    for e in errors:
        print(e, file=sys.stderr)
    sys.exit(1 if errors else 0)


if __name__ == "__main__":
    main()
