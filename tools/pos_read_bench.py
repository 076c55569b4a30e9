"""Checkable reads of one stored file (default 1 GiB at the default PoS dims); not the bench.py metric.
Writes profiles/pos_read.json and prints a summary line.

The file is written once (FileHandler.create_from_unencoded_file, chunk_cache=True); a second handler
attached to the same files without a cache is the server that keeps none.  For each read -- one row,
1 MiB, 64 MiB and the whole file, 256 columns drawn from a seed -- the run reports

  server      FileHandler.read_opening_response with and without the cache, alternating
  client      pos.client_verify_read, and the kernel regions of one call (lcpc_prof_*: HIP events)
  bytes       the rows message and the opening (arithmetic from the dims; the tests assert it)

beside the whole-column composition that was the only one available before: FileHandler.
read_full_columns (the server), then on the client the columns' canonical values brought to Montgomery
limbs (as FileHandler.polynomial_evaluation_response does it, Python integers -- timed on its own and
kept out of the totals compared), pos.client_online_verify_column_paths, and the rows read encoded
and compared at the opened columns as pos.client_verify_update_evaluation does.  New and earlier code
alternate in one run; call times are host clocks around calls that end in a device synchronise, the
median of --reps after a warm-up call.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ENCODE_BATCH_ROWS = 512   # rows per encode_rows call of the earlier composition (128 MiB of codeword)


def summary(ts):
    return {"times_s": [round(x, 6) for x in ts], "median_s": round(statistics.median(ts), 6),
            "spread_s": round(max(ts) - min(ts), 6)}


def timed_alternating(fns, reps):
    """Each of fns once per round, reps + 1 rounds, the first (warm-up) round dropped."""
    ts = [[] for _ in fns]
    for _ in range(reps + 1):
        for fn, t in zip(fns, ts):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    return [summary(t[1:] or t) for t in ts]


def regions(lcpc2d, fn):
    """{region: ms per call} of one call of fn (the library's HIP-event regions)."""
    lcpc2d.prof_enable(True)
    lcpc2d.prof_reset()
    fn()
    out = {k: round(ms, 4) for k, (ms, n) in sorted(lcpc2d.prof_stats().items()) if n}
    lcpc2d.prof_enable(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--dir", default=None, help="where the stored files go (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_read.json"))
    a = ap.parse_args()

    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import lcpc2d, pos as P, pos_files as PF
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    n_bytes = a.mib << 20
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(n_bytes)
    rb = 7 * pre
    work = tempfile.mkdtemp(prefix="pos_read_bench_", dir=a.dir)
    result = {"tool": "tools/pos_read_bench.py", "mib": a.mib, "reps": a.reps, "pre": pre, "enc": enc,
              "n_columns": a.columns, "reads": {}, "not_measured": []}
    try:
        data = np.random.default_rng(a.seed).integers(0, 256, n_bytes, dtype=np.uint8).tobytes()
        raw = os.path.join(work, "file.bin")
        with open(raw, "wb") as f:
            f.write(data)
        ulid = "01READBENCH" + "0" * 15
        t0 = time.perf_counter()
        cached = PF.FileHandler.create_from_unencoded_file(ulid, raw, pre, enc, directory=work, chunk_cache=True)
        result["create_s"] = round(time.perf_counter() - t0, 3)
        plain = PF.FileHandler.new_attach_to_existing_ulid(work, ulid, chunk_cache=False)
        rows = cached.rows_written
        result["n_rows"] = rows
        root = cached.get_commit_root()
        cols = sorted(int(c) for c in np.random.default_rng(a.seed + 1).choice(enc, size=a.columns, replace=False))
        code = lcpc2d.LigeroEncoding.new_from_dims(0, pre, enc)
        path_len = enc.bit_length() - 1
        mid = (rows // 2) * rb
        reads = {"one_row": (mid + 5, mid + rb - 5), "1MiB": (mid + 5, mid + 5 + (1 << 20)),
                 "64MiB": (mid + 5, min(mid + 5 + (64 << 20), n_bytes)), "whole_file": (0, n_bytes)}
        for name, (lo, hi) in reads.items():
            plan = P.read_plan(n_bytes, lo, hi, pre)
            rows_msg = cached.read_rows_response(lo, hi)
            got = {}

            def server_cached():
                got["opening"] = cached.read_opening_response(lo, hi, cols)

            def server_plain():
                got["plain"] = plain.read_opening_response(lo, hi, cols)

            def server_earlier():
                got["columns"] = plain.read_full_columns(cols)

            t_cached, t_plain, t_earlier_server = timed_alternating([server_cached, server_plain, server_earlier], a.reps)
            opening = got["opening"]
            assert np.array_equal(opening.segments, got["plain"].segments) and \
                np.array_equal(opening.covers, got["plain"].covers), "the two servers differ"

            def client():
                got["bytes"] = P.client_verify_read(root, n_bytes, pre, enc, lo, hi, rows_msg, cols, opening)

            # the earlier composition's client: the Montgomery limbs once (timed apart), then paths and rows
            t0 = time.perf_counter()
            mont = [lcpc2d.LcColumn(np.array([(int(v) << 64) % P.FT63_MODULUS for v in np.asarray(c.col).reshape(-1)],
                                             np.uint64).reshape(-1, 1), c.path) for c in got["columns"]]
            t_convert = time.perf_counter() - t0

            def client_earlier():
                P.client_online_verify_column_paths(root, cols, mont)
                n = plan.row_hi - plan.row_lo
                for r0 in range(0, n, ENCODE_BATCH_ROWS):
                    r1 = min(n, r0 + ENCODE_BATCH_ROWS)
                    m = np.zeros((r1 - r0, enc, 1), np.uint64)
                    for i in range(r0, r1):
                        el = P.convert_byte_vec_to_field_elements_vec(rows_msg[i * rb:(i + 1) * rb])
                        m[i - r0, :el.shape[0]] = el
                    m = code.encode_rows(m)
                    for k, c in enumerate(cols):
                        col = np.asarray(mont[k].col).reshape(-1)
                        assert np.array_equal(m[:, c, 0], col[plan.row_lo + r0:plan.row_lo + r1]), "rows mismatch"

            t_client, t_client_earlier = timed_alternating([client, client_earlier], a.reps)
            assert got["bytes"] == data[lo:hi]
            seg_rows = plan.seg_row_hi - plan.seg_row_lo
            want = len(cols) * (8 * seg_rows + 32 * plan.n_cover + 32 * path_len)
            assert opening.n_bytes() == want
            result["reads"][name] = {
                "byte_range": [lo, hi], "rows_read": plan.row_hi - plan.row_lo, "chunks": [plan.chunk_lo, plan.chunk_hi],
                "segment_rows": seg_rows, "n_cover": plan.n_cover,
                "rows_message_bytes": len(rows_msg), "opening_bytes": want,
                "earlier_opening_bytes": len(cols) * (8 * rows + 32 * path_len),
                "server_cached": t_cached, "server_no_cache": t_plain, "server_earlier_read_full_columns": t_earlier_server,
                "client_verify_read": t_client, "client_earlier_paths_and_rows": t_client_earlier,
                "client_earlier_to_montgomery_s": round(t_convert, 6),
                "client_kernel_regions_ms": regions(lcpc2d, client),
                "server_cached_kernel_regions_ms": regions(lcpc2d, server_cached),
                "server_no_cache_kernel_regions_ms": regions(lcpc2d, server_plain),
            }
            print(name, json.dumps({k: (v["median_s"] if isinstance(v, dict) and "median_s" in v else v)
                                    for k, v in result["reads"][name].items()}), flush=True)
        result["not_measured"] += ["other dims and column counts", "files above 1 GiB (thousands of chunks per column)",
                                   "the network: byte counts are arithmetic from the dims"]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"server_cached_s": v["server_cached"]["median_s"],
                          "server_no_cache_s": v["server_no_cache"]["median_s"],
                          "client_s": v["client_verify_read"]["median_s"], "opening_bytes": v["opening_bytes"]}
                      for k, v in result["reads"].items()}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
