"""The update audit's evaluations on one file image (default 1 GiB at the default PoS dims); not the
bench.py metric.  Writes profiles/pos_update.json and prints a summary line.

Stages, each in a child process of its own under a time limit (a failing stage ends the run):
  copy       the box's copy rate: device-to-device copies of the image, bytes read + written per second
  eval       lcpc_pos_eval_poly_bytes_device and lcpc_pos_eval_poly_bytes (host image) against the
             composition the wrapper was before this feature (lcpc_pos_side_vectors brought to the
             host + a one-column collapse over the packed elements), same data, same words
  left       lcpc_pos_left_multiply_bytes[_device] against the earlier composition (the host's numpy
             element image + lcpc_collapse_columns), same words
  audit      lcpc_pos_update_evaluation against its parts in turn (two lcpc_pos_commit_eval_bytes_device,
             two lcpc_open_columns), alternating
Call times are host clocks around calls that end in a device synchronise, median of --reps after a
warm-up; kernel times are the library's HIP-event regions (lcpc_prof_*), the mean of five further
repeats.  The
kernels' rate is the image's bytes over the region time, and `of_copy_rate` is that over the copy
stage's rate.
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

STAGES = {"copy": 300, "eval": 600, "left": 600, "audit": 600}   # time limit per stage, seconds
u64p = C.POINTER(C.c_uint64)


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):           # the first run warms the pools and is dropped
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return summary(ts[1:] or ts)


def summary(ts):
    return {"times_s": [round(x, 7) for x in ts], "median_s": round(statistics.median(ts), 7),
            "spread_s": round(max(ts) - min(ts), 7)}


def timed_alternating(fa, fb, reps):
    ta, tb = [], []
    for _ in range(reps + 1):
        for fn, ts in ((fa, ta), (fb, tb)):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
    return [summary(ts[1:] or ts) for ts in (ta, tb)]


class Hip:
    """Device buffers through the HIP runtime the library links."""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so.7")
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipFree.argtypes = [C.c_void_p]

    def alloc(self, n):
        p = C.c_void_p()
        assert self.L.hipMalloc(C.byref(p), n) == 0, "hipMalloc"
        return p.value

    def upload(self, a):
        p = self.alloc(a.nbytes + 16)
        assert self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0, "hipMemcpy"
        return p

    def d2d(self, dst, src, n):
        assert self.L.hipMemcpy(dst, src, n, 3) == 0, "hipMemcpy"

    def sync(self):
        assert self.L.hipDeviceSynchronize() == 0


def ok(rc, N):
    if rc:
        raise RuntimeError(f"status {rc}: {N.last_error()}")


def region_ms(lcpc2d, name, fn):
    lcpc2d.prof_enable(True)
    lcpc2d.prof_reset()
    for _ in range(5):
        fn()
    ms, count = lcpc2d.prof_stats().get(name, (0.0, 0))
    lcpc2d.prof_enable(False)
    return ms / count if count else 0.0


def stage(name, n_bytes, reps, seed):
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos as P
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    lib, hip = N.load(), Hip()
    data = np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)
    x = lcpc2d.field_random(0, 1, 1337).reshape(-1)
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(n_bytes)
    n_el = -(-n_bytes // 7)
    n_rows = -(-n_el // pre)
    res = {"n_bytes": n_bytes, "pre": pre, "enc": enc, "n_rows": n_rows}
    if name == "copy":
        a, b = hip.upload(data), hip.alloc(n_bytes + 16)
        k = 20   # copies per timed window

        def copies():
            for _ in range(k):
                hip.d2d(b, a, n_bytes)
            hip.sync()
        t = timed(copies, max(reps, 5))
        res.update(window=t, copies_per_window=k, bytes_moved_per_copy=2 * n_bytes,
                   rate_gb_s=round(k * 2 * n_bytes / t["median_s"] / 1e9, 1))
    elif name == "eval":
        d = hip.upload(data)
        out_d, out_h, px = np.zeros(1, np.uint64), np.zeros(1, np.uint64), x.ctypes.data_as(u64p)
        dev = lambda: ok(lib.lcpc_pos_eval_poly_bytes_device(d, n_bytes, px, 0, out_d.ctypes.data_as(u64p)), N)  # noqa: E731
        host = lambda: ok(lib.lcpc_pos_eval_poly_bytes(data.ctypes.data, n_bytes, px, 0, out_h.ctypes.data_as(u64p)), N)  # noqa: E731
        el = P.convert_byte_vec_to_field_elements_vec(data.tobytes())
        before = {}

        def earlier():  # pos.evaluate_field_polynomial_at_point before this feature
            _, right = P.form_side_vectors_for_polynomial_evaluation_from_point(x, 1, n_el)
            before["v"] = P.field_dot(el, right)
        t_dev = timed(dev, reps)
        t_host, t_before = timed_alternating(host, earlier, reps)
        assert out_d[0] == out_h[0] == before["v"].reshape(-1)[0], "the three evaluations differ"
        ms = region_ms(lcpc2d, "pos_poly_eval", dev)
        res.update(device_call=t_dev, host_call=t_host, earlier_composition=t_before, kernel_ms=round(ms, 4),
                   kernel_rate_gb_s=round(n_bytes / (ms / 1e3) / 1e9, 1) if ms else None,
                   speedup_host_vs_earlier=round(t_before["median_s"] / t_host["median_s"], 1))
    elif name == "left":
        d = hip.upload(data)
        left, _ = P.form_side_vectors_for_polynomial_evaluation_from_point(x, n_rows, pre)
        left = np.ascontiguousarray(left.reshape(-1))
        out_d, out_h, before = np.zeros(pre, np.uint64), np.zeros(pre, np.uint64), {}
        pl = left.ctypes.data_as(u64p)
        dev = lambda: ok(lib.lcpc_pos_left_multiply_bytes_device(d, n_bytes, pre, pl, n_rows, out_d.ctypes.data_as(u64p)), N)  # noqa: E731
        host = lambda: ok(lib.lcpc_pos_left_multiply_bytes(data.ctypes.data, n_bytes, pre, pl, n_rows, out_h.ctypes.data_as(u64p)), N)  # noqa: E731
        raw = data.tobytes()

        def earlier():  # pos.left_multiply_unencoded_matrix_by_vector before this feature
            el = P.convert_byte_vec_to_field_elements_vec(raw).reshape(-1)
            m = np.zeros(n_rows * pre, np.uint64)
            m[:el.size] = el
            before["v"] = lcpc2d.collapse_columns(0, m, left, n_rows, pre)
        t_dev = timed(dev, reps)
        t_host, t_before = timed_alternating(host, earlier, reps)
        assert np.array_equal(out_d, out_h) and np.array_equal(out_h, before["v"].reshape(-1)), "results differ"
        ms = region_ms(lcpc2d, "pos_left_mul_bytes", dev)
        res.update(device_call=t_dev, host_call=t_host, earlier_composition=t_before, kernel_ms=round(ms, 4),
                   kernel_rate_gb_s=round(n_bytes / (ms / 1e3) / 1e9, 1) if ms else None,
                   speedup_host_vs_earlier=round(t_before["median_s"] / t_host["median_s"], 1))
    elif name == "audit":
        new = data.copy()
        new[7 * pre - 3:7 * pre + 8] ^= 0x5A        # an edit across the first row boundary
        d_old, d_new = hip.upload(data), hip.upload(new)
        code = lcpc2d.LigeroEncoding.new_from_dims(0, pre, enc)
        cols = sorted(P.get_column_indicies_from_random_seed(7, 309, enc))
        fused = {}

        def audit():
            fused["v"] = P._update_evaluation(code, d_old, n_bytes, code, d_new, n_bytes, x, cols, cols, False)

        left, _ = P.form_side_vectors_for_polynomial_evaluation_from_point(x, n_rows, pre)
        parts = {}

        def in_parts():
            for key, d in (("old", d_old), ("new", d_new)):
                c, ev = lcpc2d.LcCommit.commit_pos_bytes_device_eval(d, n_bytes, code, left)
                parts[key] = (ev, c.open_columns(cols), c.get_root())
                del c
        t_audit, t_parts = timed_alternating(audit, in_parts, reps)
        for i, key in enumerate(("old", "new")):
            assert np.array_equal(fused["v"][i][0], parts[key][0]) and fused["v"][i][2] == parts[key][2]
        res.update(update_evaluation=t_audit, parts_in_turn=t_parts, n_columns=len(cols),
                   ratio=round(t_audit["median_s"] / t_parts["median_s"], 3))
    else:
        raise SystemExit(f"unknown stage {name}")
    print("STAGE_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--stage", choices=sorted(STAGES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_update.json"))
    a = ap.parse_args()
    if a.stage:
        return stage(a.stage, a.mib << 20, a.reps, a.seed)
    result = {"tool": "tools/pos_update_bench.py", "mib": a.mib, "reps": a.reps, "stages": {}, "not_measured": []}
    for name, limit in STAGES.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--stage", name, "--mib", str(a.mib), "--reps", str(a.reps),
               "--seed", str(a.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            result["not_measured"] += [f"{name}: exceeded its {limit} s limit"] + \
                [f"{s}: not run" for s in list(STAGES)[list(STAGES).index(name) + 1:]]
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("STAGE_RESULT ")]
        if r.returncode or not line:
            result["not_measured"] += [f"{name}: exit {r.returncode}: {r.stderr.strip()[-400:]}"] + \
                [f"{s}: not run" for s in list(STAGES)[list(STAGES).index(name) + 1:]]
            break
        result["stages"][name] = json.loads(line[0][len("STAGE_RESULT "):])
    st = result["stages"]
    if "copy" in st:
        for k in ("eval", "left"):
            if k in st and st[k].get("kernel_rate_gb_s"):
                st[k]["of_copy_rate"] = round(st[k]["kernel_rate_gb_s"] / st["copy"]["rate_gb_s"], 3)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {kk: v for kk, v in s.items() if not isinstance(v, dict)} for k, s in st.items()}
                     | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
