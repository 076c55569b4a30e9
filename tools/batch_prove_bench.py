"""Batched evaluation proofs against m single proofs, and the many-tensor row combination alone;
not the bench.py metric.  Writes profiles/batch_prove.json and prints a summary line.

Shape: Ft127, 2^24 coefficients, Ligero at rho = 1/2 (512 x 32768 -> 65536).  For m in {1, 4, 16, 64}:
  prove_batch / verify_batch   wall time of LcCommit.prove_batch and LcBatchEvalProof.verify, `--reps`
                               timed runs after `--warmup`: median and spread (max - min);
  sequential                   m LcCommit.prove / LcEvalProof.verify calls on the same commitment and
                               tree, timed the same way;
  bytes                        the serialized batch proof against m serialized single proofs.
The kernel alone (lcpc_collapse_columns_many; the time is that of its two launches, taken with HIP
events by the library's profiler, regions collapse_many_partial + collapse_many_fold) at T in
{8, 16, 64} over the same 512 x 32768 matrix, in this process (the default kernels) and in a child
with LCPC_NO_MFMA=1 (the VALU kernel), plus one Ft255 line.  Each is set against two floors measured
in the same run:
  read floor       one read of the coefficient matrix at the copy rate: a device-to-device copy of the
                   matrix's size, its rate counted over the bytes read plus the bytes written;
  multiply floor   T x n_rows x n_per_row Montgomery products at the field's multiply rate as
                   tools/microbench/femul2 measures it (built beforehand: make -C tools/microbench
                   femul2; run here as a child before this process touches the GPU).
--bench-lines FILE embeds parent / child bench.py result lines gathered on the same machine.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
FT127, FT255 = 1, 3
LOG_LEN = 24


def med_spread(xs):
    return {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "runs_ms": xs}


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return med_spread(out)


def femul_rates(path):
    """{field: G mul/s} of the library's product from tools/microbench/femul2 (a child process)"""
    if not os.path.exists(path):
        return None
    r = subprocess.run([path], capture_output=True, text=True, timeout=120)
    if r.returncode:
        return None
    rates = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(Ft\d+)\s+library\s+[\d.]+ ms\s+([\d.]+) G mul/s", line)
        if m:
            rates[m.group(1)] = float(m.group(2))
    return rates or None


def copy_rate_gbs(nbytes, reps=5):
    """GB/s (bytes read + bytes written) of a device-to-device copy of nbytes, HIP events around it"""
    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    a, b, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    if hip.hipMalloc(C.byref(a), nbytes) or hip.hipMalloc(C.byref(b), nbytes):
        raise RuntimeError("hipMalloc failed")
    hip.hipEventCreate(C.byref(e0))
    hip.hipEventCreate(C.byref(e1))
    ms = []
    for _ in range(reps + 1):
        hip.hipEventRecord(e0, None)
        hip.hipMemcpyAsync(b, a, nbytes, 3, None)
        hip.hipEventRecord(e1, None)
        hip.hipEventSynchronize(e1)
        t = C.c_float()
        hip.hipEventElapsedTime(C.byref(t), e0, e1)
        ms.append(t.value)
    hip.hipFree(a)
    hip.hipFree(b)
    best = statistics.median(ms[1:])
    return 2 * nbytes / (best * 1e-3) / 1e9


def kernel_times(L, fid, n_rows, n_per_row, ts, reps):
    """{T: median / spread of the two launches' device time} for random inputs"""
    coeffs = L.field_random(fid, n_rows * n_per_row, 3)
    out = {}
    L.prof_enable(True)
    for t in ts:
        tens = L.field_random(fid, t * n_rows, 4 + t).reshape(t, n_rows, -1)
        runs = []
        for rep in range(reps + 1):
            L.prof_reset()
            L.collapse_columns_many(fid, coeffs, tens, n_rows, n_per_row)
            st = L.prof_stats()
            runs.append(sum(st[k][0] for k in st if k.startswith("collapse_")))
        out[str(t)] = med_spread(runs[1:])
    L.prof_enable(False)
    return out


def child_kernel_times(args):
    """this tool's --kernel-only mode in a child with LCPC_NO_MFMA=1 (read once per process)"""
    env = dict(os.environ, LCPC_NO_MFMA="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--reps", str(args.reps)],
                       env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise RuntimeError("kernel-only child failed: " + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ms", default="1,4,16,64")
    ap.add_argument("--femul", default=os.path.join(HERE, "tools", "microbench", "femul2"))
    ap.add_argument("--bench-lines", help="JSON file {parent: [...], child: [...]} of bench.py result lines")
    ap.add_argument("--kernel-only", action="store_true", help="print the kernel times as one JSON line and exit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "batch_prove.json"))
    args = ap.parse_args()
    n_rows, n_per_row = 512, 32768
    ts = [8, 16, 64]
    if args.kernel_only:
        import lcpc_proof_of_storage_amd as L
        L.set_device(0)
        print(json.dumps({"Ft127": kernel_times(L, FT127, n_rows, n_per_row, ts, args.reps),
                          "Ft255": kernel_times(L, FT255, n_rows, n_per_row, [16], args.reps)}))
        return
    mul_rates = femul_rates(args.femul)  # before this process opens the GPU
    valu = child_kernel_times(args)
    import lcpc_proof_of_storage_amd as L
    L.set_device(0)
    n = 1 << LOG_LEN
    enc = L.LigeroEncoding.new(FT127, n)
    assert (enc.n_per_row, enc.n_cols) == (n_per_row, 65536)
    coeffs = L.field_random(FT127, n, 1)
    comm = L.LcCommit.commit(coeffs, enc)
    root = comm.get_root()

    def tr():
        t = L.Transcript(b"batch bench")
        t.append_message(b"polycommit", root)
        return t

    res = {"shape": {"field": "Ft127", "log_len": LOG_LEN, "n_rows": n_rows, "n_per_row": n_per_row,
                     "n_cols": enc.n_cols, "n_col_opens": enc.get_n_col_opens(),
                     "n_degree_tests": enc.get_n_degree_tests()},
           "reps": args.reps, "warmup": args.warmup, "by_m": {}}
    for m in [int(x) for x in args.ms.split(",")]:
        outers = np.ascontiguousarray(L.field_random(FT127, m * n_rows, 10 + m).reshape(m, n_rows, -1))
        inners = np.ascontiguousarray(L.field_random(FT127, m * n_per_row, 20 + m).reshape(m, n_per_row, -1))
        batch = comm.prove_batch(outers, enc, tr())
        singles = [comm.prove(outers[j], enc, tr()) for j in range(m)]
        evs = batch.verify(root, outers, inners, enc, tr())
        for j in range(m):  # the batch's evaluations are the single proofs'
            assert np.array_equal(evs[j], singles[j].verify(root, outers[j], inners[j], enc, tr())), j
        row = {
            "prove_batch": timed(lambda: comm.prove_batch(outers, enc, tr()), args.reps, args.warmup),
            "prove_sequential": timed(lambda: [comm.prove(outers[j], enc, tr()) for j in range(m)], args.reps,
                                      args.warmup),
            "verify_batch": timed(lambda: batch.verify(root, outers, inners, enc, tr()), args.reps, args.warmup),
            "verify_sequential": timed(lambda: [singles[j].verify(root, outers[j], inners[j], enc, tr())
                                                for j in range(m)], args.reps, args.warmup),
            "bytes_batch": len(batch.to_bytes()),
            "bytes_sequential": m * len(singles[0].to_bincode()),
        }
        for k in ("prove", "verify"):
            b, s = row[k + "_batch"], row[k + "_sequential"]
            row[k + "_batched_below_sequential"] = b["median_ms"] + b["spread_ms"] < s["median_ms"]
            row[k + "_speedup"] = s["median_ms"] / b["median_ms"]
        res["by_m"][str(m)] = row
        del batch, singles
    # the kernel alone, against its floors
    default = {"Ft127": kernel_times(L, FT127, n_rows, n_per_row, ts, args.reps),
               "Ft255": kernel_times(L, FT255, n_rows, n_per_row, [16], args.reps)}
    copy_gbs = copy_rate_gbs(n_rows * n_per_row * 16)
    kern = {"copy_rate_gbs": copy_gbs, "mul_rates_gmuls": mul_rates,
            "mul_rate_source": "tools/microbench/femul2, this run" if mul_rates else "not measured (femul2 not built)",
            "rows": []}
    for field, fb in (("Ft127", 16), ("Ft255", 32)):
        for t, d in default[field].items():
            t = int(t)
            rate = (mul_rates or {}).get(field)
            kern["rows"].append({
                "field": field, "T": t, "default_kernel": d, "valu_kernel": valu[field][str(t)],
                "read_floor_ms": n_rows * n_per_row * fb / (copy_gbs * 1e9) * 1e3,
                "multiply_floor_ms": t * n_rows * n_per_row / (rate * 1e9) * 1e3 if rate else None})
    res["kernel"] = kern
    if args.bench_lines:
        res["bench_py"] = json.load(open(args.bench_lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({m: {k: round(v["median_ms"], 3) if isinstance(v, dict) else v for k, v in r.items()}
                      for m, r in res["by_m"].items()}))
    print(json.dumps(kern["rows"]))


if __name__ == "__main__":
    main()
