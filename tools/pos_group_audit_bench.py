"""Grouped audits of stored files: u^T M for a whole fleet of files in one call
(lcpc_pos_left_multiply_bytes_grouped[_device]) against one lcpc_pos_left_multiply_bytes[_device]
call per file, the parent's behaviour, in the same process; not the bench.py metric.  Writes
profiles/pos_group_audit.json and prints a summary line.

Fleets, each in a child process of its own under a time limit (a failing stage ends the run), all at
the default PoS dims of their file size:
  1mib_x1024, 64kib_x4096, 16mib_x64   equal-sized files
  mixed                                 2048 x 64 KiB, 256 x 1 MiB and 8 x 16 MiB, shuffled
  e2e                                   pos_files.answer_evaluation_requests against a loop of
                                        FileHandler.polynomial_evaluation_response over 256 stored files
                                        of 64 KiB, with the old loop's Python conversion timed apart
For a fleet: the wall time of the call from host memory and from a device arena, and the device time
of the call's launches (the library's HIP-event regions: pos_group_left_mul for the grouped call,
pos_left_mul_bytes for the single calls), each the median of --reps (5) after one warm-up; the spread
is max - min.  The single calls' count is the fleet's file count, never taken from the grouped code.
The results are compared word for word.  Verdict per figure: the grouped median plus its
spread is below the singles' median.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KIB, MIB = 1 << 10, 1 << 20
FLEETS = {
    "1mib_x1024": [(MIB, 1024)],
    "64kib_x4096": [(64 * KIB, 4096)],
    "16mib_x64": [(16 * MIB, 64)],
    "mixed": [(64 * KIB, 2048), (MIB, 256), (16 * MIB, 8)],
}
E2E_FILES, E2E_BYTES = 256, 64 * KIB
LIMIT_S = 420   # per stage
u64p = C.POINTER(C.c_uint64)
szp = C.POINTER(C.c_size_t)


def summary(ts, unit):
    return {f"times_{unit}": [round(x, 5) for x in ts], f"median_{unit}": round(statistics.median(ts), 5),
            f"spread_{unit}": round(max(ts) - min(ts), 5)}


def wall(fn, reps):
    ts = []
    for _ in range(reps + 1):            # the first run warms the pools and is dropped
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return summary(ts[1:], "s")


def regions_ms(lcpc2d, names, fn, reps):
    """(device time, launches) of the named regions per call of fn, after a warm-up"""
    ts, counts = [], []
    lcpc2d.prof_enable(True)
    for _ in range(reps + 1):
        lcpc2d.prof_reset()
        fn()
        st = lcpc2d.prof_stats()
        ts.append(sum(st.get(n, (0.0, 0))[0] for n in names))
        counts.append(sum(st.get(n, (0.0, 0))[1] for n in names))
    lcpc2d.prof_enable(False)
    lcpc2d.prof_reset()
    return summary(ts[1:], "ms") | {"regions": counts[-1]}


def verdict(grouped, singles, unit):
    g, s = grouped[f"median_{unit}"], singles[f"median_{unit}"]
    return {"singles_over_grouped": round(s / g, 2) if g else None,
            "grouped_wins": g + grouped[f"spread_{unit}"] < s}


def ok(rc, N):
    if rc:
        raise RuntimeError(f"status {rc}: {N.last_error()}")


def fleet_stage(name, reps, seed):
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos as P
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    lib = N.load()
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.full(n, b, np.int64) for b, n in FLEETS[name]])
    rng.shuffle(sizes)
    n_jobs = sizes.size
    pres = np.array([P.get_aspect_ratio_default_from_file_len(int(b))[0] for b in sizes], np.int64)
    rows = np.array([-(-(-(-int(b) // 7)) // int(p)) for b, p in zip(sizes, pres)], np.int64)
    offsets = np.concatenate([[0], np.cumsum((sizes + 7) & ~7)[:-1]]).astype(np.int64)
    total = int(offsets[-1] + sizes[-1])
    arena = rng.integers(0, 256, total, dtype=np.uint8)
    lefts = rng.integers(0, P.FT63_MODULUS, int(rows.sum()), dtype=np.uint64)
    l_off = np.concatenate([[0], np.cumsum(rows)[:-1]])
    o_off = np.concatenate([[0], np.cumsum(pres)[:-1]])
    out_g, out_s = np.zeros(int(pres.sum()), np.uint64), np.zeros(int(pres.sum()), np.uint64)
    tiles, launches = P.left_multiply_group_plan(sizes, pres)
    res = {"files": {str(b): n for b, n in FLEETS[name]}, "n_jobs": int(n_jobs), "bytes": total,
           "pre": sorted({int(p) for p in pres}), "plan": {"launches": int(launches), "tiles": int(tiles.size),
                                                           "single_path_jobs": int((tiles["launch"] == P.GROUP_SINGLE).sum())}}
    c_sizes, c_pres, c_off = (np.ascontiguousarray(a, np.uint64).astype(C.c_size_t) for a in (sizes, pres, offsets))
    sp = lambda a: a.ctypes.data_as(szp)  # noqa: E731
    pl, pg, ps = lefts.ctypes.data_as(u64p), out_g.ctypes.data_as(u64p), out_s.ctypes.data
    host_ptrs = (C.c_void_p * n_jobs)(*[arena.ctypes.data + int(o) for o in offsets])
    job_args = [(int(offsets[j]), int(sizes[j]), int(pres[j]), C.cast(lefts.ctypes.data + 8 * int(l_off[j]), u64p),
                 int(rows[j]), C.cast(ps + 8 * int(o_off[j]), u64p)) for j in range(n_jobs)]

    def grouped_host():
        ok(lib.lcpc_pos_left_multiply_bytes_grouped(host_ptrs, sp(c_sizes), sp(c_pres), n_jobs, pl, lefts.size, pg,
                                                    out_g.size), N)

    def singles_host():
        base = arena.ctypes.data
        for off, nb, pre, lp, nr, op in job_args:
            ok(lib.lcpc_pos_left_multiply_bytes(base + off, nb, pre, lp, nr, op), N)

    res["host"] = {"grouped": wall(grouped_host, reps), "singles": wall(singles_host, reps)}
    assert np.array_equal(out_g, out_s), "the grouped host entry differs from the single calls"
    res["host"]["wall"] = verdict(res["host"]["grouped"], res["host"]["singles"], "s")

    hip = C.CDLL("libamdhip64.so.7")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), total + 64) == 0 and hip.hipMemcpy(d, arena.ctypes.data, total, 1) == 0
    out_g[:] = 0
    out_s[:] = 0

    def grouped_device():
        ok(lib.lcpc_pos_left_multiply_bytes_grouped_device(d.value, sp(c_off), sp(c_sizes), sp(c_pres), n_jobs, pl,
                                                           lefts.size, pg, out_g.size), N)

    def singles_device():
        for off, nb, pre, lp, nr, op in job_args:
            ok(lib.lcpc_pos_left_multiply_bytes_device(d.value + off, nb, pre, lp, nr, op), N)

    dev = res["device"] = {"grouped": wall(grouped_device, reps), "singles": wall(singles_device, reps)}
    assert np.array_equal(out_g, out_s), "the grouped device entry differs from the single calls"
    dev["wall"] = verdict(dev["grouped"], dev["singles"], "s")
    dev["grouped_device_time"] = regions_ms(lcpc2d, ("pos_group_left_mul",), grouped_device, reps)
    dev["singles_device_time"] = regions_ms(lcpc2d, ("pos_left_mul_bytes",), singles_device, reps)
    dev["device_time"] = verdict(dev["grouped_device_time"], dev["singles_device_time"], "ms")
    print("STAGE_RESULT " + json.dumps(res))


def e2e_stage(reps, seed):
    import tempfile
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import pos as P, pos_files as PF
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    rng = np.random.default_rng(seed)
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(E2E_BYTES)
    n_open = min(P.get_PoS_soudness_n_cols(pre, enc), enc)
    points = L.field_random(0, E2E_FILES, seed)
    with tempfile.TemporaryDirectory() as tmp:
        requests = []
        for i in range(E2E_FILES):
            name = f"01BENCH{i:019d}"
            src = os.path.join(tmp, name + ".bin")
            with open(src, "wb") as f:
                f.write(rng.integers(0, 256, E2E_BYTES, dtype=np.uint8).tobytes())
            fh = PF.FileHandler.create_from_unencoded_file(name, src, pre, enc, directory=os.path.join(tmp, name))
            cols = sorted(rng.choice(enc, size=n_open, replace=False).tolist())
            requests.append((fh, points[i:i + 1], cols))
        got, want = [], []

        def grouped():
            got[:] = PF.answer_evaluation_requests(requests)

        def loop():
            want[:] = [fh.polynomial_evaluation_response(x, cols) for fh, x, cols in requests]

        opened = [fh.read_full_columns(cols) for fh, _, cols in requests]

        def conversion():   # the per-element expression of polynomial_evaluation_response, alone
            for cs in opened:
                for c in cs:
                    np.array([(int(v) << 64) % P.FT63_MODULUS for v in np.asarray(c.col).reshape(-1)], np.uint64)

        res = {"files": E2E_FILES, "file_bytes": E2E_BYTES, "pre": pre, "enc": enc, "opened_columns": n_open,
               "grouped": wall(grouped, reps), "loop": wall(loop, reps), "loop_python_conversion": wall(conversion, reps)}
        for (r1, c1), (r2, c2) in zip(got, want):
            assert np.array_equal(r1, r2) and all(np.array_equal(a.col, b.col) and a.path == b.path for a, b in zip(c1, c2))
    res["wall"] = verdict(res["grouped"], res["loop"], "s")
    res["conversion_share_of_loop"] = round(res["loop_python_conversion"]["median_s"] / res["loop"]["median_s"], 3)
    rest = res["loop"]["median_s"] - res["loop_python_conversion"]["median_s"]
    res["loop_without_conversion_over_grouped"] = round(rest / res["grouped"]["median_s"], 2)
    print("STAGE_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", nargs="+", default=list(FLEETS) + ["e2e"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--stage")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_group_audit.json"))
    a = ap.parse_args()
    if a.stage:
        return e2e_stage(a.reps, a.seed) if a.stage == "e2e" else fleet_stage(a.stage, a.reps, a.seed)
    result = {"tool": "tools/pos_group_audit_bench.py", "reps": a.reps, "fleets": {}, "not_measured": []}
    for name in a.fleets:
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--reps", str(a.reps), "--seed", str(a.seed)]
        print(f"stage {name} ...", file=sys.stderr, flush=True)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            result["not_measured"].append(f"{name}: exceeded its {LIMIT_S} s limit")
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STAGE_RESULT ")]
        if r.returncode or not line:
            result["not_measured"].append(f"{name}: exit {r.returncode}: {r.stderr.strip()[-400:]}")
            break
        result["fleets"][name] = json.loads(line[0][len("STAGE_RESULT "):])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {}
    for name, st in result["fleets"].items():
        if name == "e2e":
            brief[name] = {"grouped_s": st["grouped"]["median_s"], "loop_s": st["loop"]["median_s"],
                           "conversion_share": st["conversion_share_of_loop"]}
        else:
            brief[name] = {"host_s": [st["host"]["grouped"]["median_s"], st["host"]["singles"]["median_s"]],
                           "device_s": [st["device"]["grouped"]["median_s"], st["device"]["singles"]["median_s"]],
                           "device_time_ms": [st["device"]["grouped_device_time"]["median_ms"],
                                              st["device"]["singles_device_time"]["median_ms"]]}
    print(json.dumps(brief | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
