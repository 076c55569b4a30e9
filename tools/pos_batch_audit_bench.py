"""Batched audits of a stored file: m left vectors against one file image in one pass
(lcpc_pos_left_multiply_bytes_many), on a 1 GiB and a 64 MiB image at the default PoS dims; not the
bench.py metric.  Writes profiles/pos_batch_audit.json and prints a summary line.

Stages, each in a child process of its own under a time limit (a failing stage ends the run):
  copy         the box's copy rate: device-to-device copies of the image, bytes read + written per second
  mfma / valu  the device entry under the default dispatch and under LCPC_NO_MFMA=1 (read once per
               process; "kernel" records what ran: the default dispatch names the matrix cores from
               POS_LEFT_MANY_MFMA_MIN_VECS vectors on, and the adoption measurement itself is taken on a
               build with that constant at 1), m in {1, 4, 16, 64}: the device time of the call's launches (the library's
               HIP-event regions pos_left_mul_many_prepare + pos_left_mul_many + pos_left_mul_many_fold),
               against m times one lcpc_pos_left_multiply_bytes_device (region pos_left_mul_bytes), the
               parent's composition, measured in the same process; the results are compared word for word
  host         the host entry's wall time against m times one single host call and against one upload
Every figure is the median of --reps (5) after one warm-up; the spread is max - min.  The adoption
rule reads the two kernel stages: the matrix cores are the default from the smallest measured m at
which, for that m and every larger one, their median plus spread is below the VALU kernel's median.
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

STAGES = {"copy": 300, "mfma": 600, "valu": 600, "host": 600}   # time limit per stage, seconds
VECS = (1, 4, 16, 64)
N_OPEN = 256                 # opened columns of one audit at the default dims
FT63_MUL_RATE_G = 1701.0     # Ft63 Montgomery products per second, tools/microbench/femul2
REGIONS = ("pos_left_mul_many_prepare", "pos_left_mul_many", "pos_left_mul_many_fold")
u64p = C.POINTER(C.c_uint64)


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


class Hip:
    """Device buffers through the HIP runtime the library links."""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so.7")
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def alloc(self, n):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), n) == 0, "hipMalloc"
        return p.value

    def upload(self, a, dst=None):
        p = dst or self.alloc(a.nbytes + 16)
        assert self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0, "hipMemcpy"
        return p

    def d2d(self, dst, src, n):
        assert self.L.hipMemcpy(dst, src, n, 3) == 0, "hipMemcpy"

    def sync(self):
        assert self.L.hipDeviceSynchronize() == 0


def ok(rc, N):
    if rc:
        raise RuntimeError(f"status {rc}: {N.last_error()}")


def regions_ms(lcpc2d, names, fn, reps):
    """device time of the named regions per call of fn: one sample per call, after a warm-up"""
    ts = []
    lcpc2d.prof_enable(True)
    for _ in range(reps + 1):
        lcpc2d.prof_reset()
        fn()
        st = lcpc2d.prof_stats()
        ts.append(sum(st.get(n, (0.0, 0))[0] for n in names))
    lcpc2d.prof_enable(False)
    return summary(ts[1:], "ms")


def stage(name, n_bytes, reps, seed):
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos as P
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    lib, hip = N.load(), Hip()
    data = np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(n_bytes)
    n_rows = -(-(-(-n_bytes // 7)) // pre)
    res = {"n_bytes": n_bytes, "pre": pre, "enc": enc, "n_rows": n_rows}
    lefts = lcpc2d.field_random(0, max(VECS) * n_rows, 1337).reshape(max(VECS), n_rows)
    pl = lefts.ctypes.data_as(u64p)
    if name == "copy":
        a, b = hip.upload(data), hip.alloc(n_bytes + 16)
        k = 20   # copies per timed window

        def copies():
            for _ in range(k):
                hip.d2d(b, a, n_bytes)
            hip.sync()
        t = wall(copies, reps)
        res.update(window=t, copies_per_window=k, rate_gb_s=round(k * 2 * n_bytes / t["median_s"] / 1e9, 1))
    elif name in ("mfma", "valu"):
        d = hip.upload(data)
        one = np.zeros(pre, np.uint64)
        single = lambda: ok(lib.lcpc_pos_left_multiply_bytes_device(d, n_bytes, pre, pl, n_rows, one.ctypes.data_as(u64p)), N)  # noqa: E731
        res["single_call"] = regions_ms(lcpc2d, ("pos_left_mul_bytes",), single, reps)
        res["by_m"] = {}
        for m in VECS:
            out = np.zeros((m, pre), np.uint64)
            many = lambda: ok(lib.lcpc_pos_left_multiply_bytes_many_device(d, n_bytes, pre, pl, m, n_rows, out.ctypes.data_as(u64p)), N)  # noqa: E731
            r = regions_ms(lcpc2d, REGIONS, many, reps)
            assert np.array_equal(out[0], one), "the many-vector entry differs from the single entry"
            r["kernel"] = P.left_multiply_many_kernel(pre, m)
            r["m_single_calls_ms"] = round(m * res["single_call"]["median_ms"], 5)
            r["products"] = m * n_rows * pre
            r["products_at_mul_rate_ms"] = round(m * n_rows * pre / FT63_MUL_RATE_G / 1e6, 5)
            res["by_m"][str(m)] = r
    elif name == "host":
        one, buf = np.zeros(pre, np.uint64), hip.alloc(n_bytes + 16)
        single = lambda: ok(lib.lcpc_pos_left_multiply_bytes(data.ctypes.data, n_bytes, pre, pl, n_rows, one.ctypes.data_as(u64p)), N)  # noqa: E731
        res["single_call"] = wall(single, reps)
        res["upload_alone"] = wall(lambda: hip.upload(data, buf), reps)
        res["by_m"] = {}
        path_len = (enc - 1).bit_length()
        columns = N_OPEN * (n_rows * 8 + path_len * 32)
        for m in VECS:
            out = np.zeros((m, pre), np.uint64)
            many = lambda: ok(lib.lcpc_pos_left_multiply_bytes_many(data.ctypes.data, n_bytes, pre, pl, m, n_rows, out.ctypes.data_as(u64p)), N)  # noqa: E731
            r = wall(many, reps)
            assert np.array_equal(out[0], one), "the many-vector entry differs from the single entry"
            r["m_single_calls_s"] = round(m * res["single_call"]["median_s"], 5)
            r["response_bytes"] = m * pre * 8 + columns
            r["m_single_responses_bytes"] = m * (enc * 8 + columns)
            res["by_m"][str(m)] = r
    else:
        raise SystemExit(f"unknown stage {name}")
    print("STAGE_RESULT " + json.dumps(res))


def adoption(mfma, valu):
    """the smallest measured m from which on the matrix cores' median + spread is below the VALU median"""
    wins = [mfma["by_m"][str(m)]["kernel"] == 2 and
            mfma["by_m"][str(m)]["median_ms"] + mfma["by_m"][str(m)]["spread_ms"] < valu["by_m"][str(m)]["median_ms"]
            for m in VECS]
    first = None
    for i in range(len(VECS) - 1, -1, -1):
        if not wins[i]:
            break
        first = VECS[i]
    return {"mfma_wins_at": dict(zip(map(str, VECS), wins)), "mfma_from_m": first}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--stage", choices=sorted(STAGES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_batch_audit.json"))
    a = ap.parse_args()
    if a.stage:
        return stage(a.stage, a.mib[0] << 20, a.reps, a.seed)
    result = {"tool": "tools/pos_batch_audit_bench.py", "reps": a.reps, "images": {}, "not_measured": []}
    for mib in a.mib:
        st = result["images"][f"{mib}_mib"] = {}
        for name, limit in STAGES.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--mib", str(mib), "--reps", str(a.reps),
                   "--seed", str(a.seed)]
            env = dict(os.environ, LCPC_NO_MFMA="1" if name == "valu" else "0")
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, env=env)
            except subprocess.TimeoutExpired:
                result["not_measured"].append(f"{mib} MiB {name}: exceeded its {limit} s limit")
                break
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("STAGE_RESULT ")]
            if r.returncode or not line:
                result["not_measured"].append(f"{mib} MiB {name}: exit {r.returncode}: {r.stderr.strip()[-400:]}")
                break
            st[name] = json.loads(line[0][len("STAGE_RESULT "):])
        if "mfma" in st and "valu" in st:
            st["adoption"] = adoption(st["mfma"], st["valu"])
            if "copy" in st:
                st["one_read_at_copy_rate_ms"] = round(st["copy"]["n_bytes"] / st["copy"]["rate_gb_s"] / 1e6, 4)
        if result["not_measured"]:
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    brief = {}
    for img, st in result["images"].items():
        brief[img] = {k: {m: v["median_ms"] for m, v in st[k]["by_m"].items()} for k in ("mfma", "valu") if k in st}
        brief[img]["adoption"] = st.get("adoption")
    print(json.dumps(brief | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
