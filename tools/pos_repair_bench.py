"""Scrub and repair of one stored proof-of-storage file (pos_files.FileHandler.scrub / repair over
lcpc_pos_scrub_porenc and lcpc_pos_repair_columns); not the bench.py metric.

The file of tools/pos_edit_bench.py (default 1 GiB at the default PoS dims) is created once.  Timed,
`--reps` times each, on the mapped `.porenc`:
  scrub                lcpc_pos_scrub_porenc against the stored leaves;
  repair_1 / repair_max
                       lcpc_pos_repair_columns (columns and digests out) with 1 and with enc - pre
                       damaged columns;
  yardstick            code from before this feature with the same two transforms per row and the
                       same traffic over the link: lcpc_pos_decode_porenc of the whole image plus
                       lcpc_pos_reencode_rows of the whole file.
Then the handler's own scrub() and repair() (1 and enc - pre damaged columns) are timed once each,
write-back included, and the result is checked (verify_all_files_agree).  One profiled repeat of
repair_max gives the region times (lcpc_prof_*) that say where the time goes.  Everything is
written to profiles/pos_repair.json; a summary line is printed.
"""
import argparse
import ctypes as C
import json
import mmap
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lcpc_proof_of_storage_amd as L  # noqa: E402
from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos as P, pos_files as PF  # noqa: E402

ULID = "01POSREPAIRBENCH0000000000"
MIB = 1 << 20


def u8(a):
    return a.ctypes.data_as(N.u8p)


def timed(fn, reps):
    ts = []
    for _ in range(reps + 1):          # the first run warms the pools and is dropped
        t = time.perf_counter()
        rc = fn()
        ts.append(time.perf_counter() - t)
        if rc:
            raise RuntimeError(f"status {rc}: {N.last_error()}")
    ts = ts[1:] or ts
    return {"times_s": [round(x, 4) for x in ts], "median_s": round(statistics.median(ts), 4),
            "spread_s": round(max(ts) - min(ts), 4)}


def damage(path, cols, cap, rows, rng):
    with open(path, "r+b") as f:
        for c in cols:
            f.seek(c * cap * 8)
            f.write(rng.integers(0, 256, rows * 8, dtype=np.uint8).tobytes())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30, help="bytes of the stored file (default 1 GiB)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_repair.json"))
    args = ap.parse_args()
    L.set_device(0)
    lib = N.load()
    n = args.size
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(n)
    work = args.dir or tempfile.mkdtemp(prefix="pos_repair_bench_")
    files = os.path.join(work, "files")
    try:
        rng = np.random.default_rng(1)
        src = os.path.join(work, "source.bin")
        with open(src, "wb") as f:
            left = n
            while left:
                k = min(left, 64 * MIB)
                f.write(rng.integers(0, 256, k, dtype=np.uint8).tobytes())
                left -= k
        t = time.perf_counter()
        fh = PF.FileHandler.create_from_unencoded_file(ULID, src, pre, enc, directory=files)
        rows, cap = fh.rows_written, fh.row_capacity
        res = {"what": "scrub and erasure repair of one stored file against a decode pass plus a re-encode pass "
                       "(the same two transforms per row and link traffic, code from before this feature)",
               "size": n, "pre": pre, "enc": enc, "rows_written": rows, "row_capacity": cap, "reps": args.reps,
               "create_s": round(time.perf_counter() - t, 3)}
        leaves = np.ascontiguousarray(fh.get_merkle_tree().digests[:enc]).reshape(-1)
        raw = np.fromfile(fh.get_raw_file_handle(), np.uint8)
        one = np.array([enc // 3], np.uint64)
        many = np.sort(rng.permutation(enc)[:enc - pre]).astype(np.uint64)
        status = np.zeros(enc, np.uint8)
        digests = np.zeros(enc * 32, np.uint8)
        nbad = C.c_size_t()
        with open(fh.get_encoded_file_handle(), "r+b") as f:
            mm = mmap.mmap(f.fileno(), cap * enc * 8)
            img = np.frombuffer(mm, np.uint8)
            out = np.zeros(rows * pre * 7, np.uint8)

            def repair(cols, want_data=False):
                k = cols.size
                co, dg = np.zeros(k * rows * 8, np.uint8), np.zeros(k * 32, np.uint8)
                rc = lib.lcpc_pos_repair_columns(u8(img), pre, enc, rows, cap, cols.ctypes.data_as(N.u64p), k, u8(co),
                                                 u8(dg), u8(out) if want_data else None)
                ok = all(np.array_equal(dg[32 * i:32 * i + 32], leaves[32 * int(c):32 * int(c) + 32])
                         for i, c in enumerate(cols))
                return rc or (0 if ok else -1)
            res["scrub"] = timed(lambda: lib.lcpc_pos_scrub_porenc(u8(img), enc, rows, cap, u8(leaves), u8(digests),
                                                                  u8(status), C.byref(nbad)), args.reps)
            assert nbad.value == 0
            res["decode_file"] = timed(lambda: lib.lcpc_pos_decode_porenc(u8(img), pre, enc, cap, 0, rows, u8(out)),
                                       args.reps)
            assert np.array_equal(out[:n], raw)
            res["reencode_file"] = timed(lambda: lib.lcpc_pos_reencode_rows(u8(raw), n, pre, enc, 0, u8(img), cap),
                                         args.reps)
            res["repair_1"] = timed(lambda: repair(one), args.reps)
            res["repair_max"] = timed(lambda: repair(many), args.reps)
            res["decode_with_erasures_max"] = timed(lambda: repair(many, True), 1)
            assert np.array_equal(out[:n], raw)
            lcpc2d.prof_enable(True)
            lcpc2d.prof_reset()
            t = time.perf_counter()
            assert repair(many) == 0
            res["repair_max_profiled"] = {
                "total_s": round(time.perf_counter() - t, 4),
                "regions_ms_count": {k: [round(ms, 3), int(cnt)] for k, (ms, cnt) in lcpc2d.prof_stats().items()}}
            lcpc2d.prof_enable(False)
            del img
            mm.close()
        yard = res["decode_file"]["median_s"] + res["reencode_file"]["median_s"]
        res["yardstick_s"] = round(yard, 4)
        res["ratio_repair_max_to_yardstick"] = round(res["repair_max"]["median_s"] / yard, 3)
        res["ratio_repair_1_to_yardstick"] = round(res["repair_1"]["median_s"] / yard, 3)
        # the handler's own calls, write-back included
        t = time.perf_counter()
        assert fh.scrub().clean
        res["handler_scrub_s"] = round(time.perf_counter() - t, 4)
        for name, cols in (("handler_repair_1_s", one), ("handler_repair_max_s", many)):
            damage(fh.get_encoded_file_handle(), [int(c) for c in cols], cap, rows, rng)
            t = time.perf_counter()
            rep = fh.repair()
            res[name] = round(time.perf_counter() - t, 4)
            assert rep.bad_columns == [int(c) for c in cols] and rep.repaired_from == "columns"
        fh.verify_all_files_agree()
        res["verify_all_files_agree"] = True
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({k: res[k] for k in ("size", "yardstick_s", "ratio_repair_max_to_yardstick",
                                              "ratio_repair_1_to_yardstick", "handler_scrub_s")}
                         | {k: res[k]["median_s"] for k in ("scrub", "repair_1", "repair_max")}))
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
