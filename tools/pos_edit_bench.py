"""Edits and appends of one stored proof-of-storage file, with and without the column chunk-CV
cache (pos_files.FileHandler(chunk_cache=...)); not the bench.py metric.

One file (default 1 GiB at the default PoS dims) is created once.  A handler with
chunk_cache=False -- the full rebuild of the tree from the whole `.porenc` after every change --
runs a one-row edit, a 1 MiB edit and a 1 MiB append, `--reps` times each; then a handler with
chunk_cache=True is attached to the same files (its cache rebuilt once, timed separately) and
runs the same operations at the same offsets.  After every incremental operation the tree is
compared with a full rebuild from the `.porenc` as it then stands (untimed).  Medians, the
spread of the repeats, the bytes each operation reads from the image (derived from the row and
chunk counts) and one profiled repeat's region times (lcpc_prof_*) go to
profiles/pos_edit_incremental.json; a summary line is printed.
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
import lcpc_proof_of_storage_amd as L  # noqa: E402
from lcpc_proof_of_storage_amd import lcpc2d, pos as P, pos_files as PF  # noqa: E402

ULID = "01POSEDITBENCH000000000000"
MIB = 1 << 20


def first_row(chunk):
    return 0 if chunk == 0 else 128 * chunk - 4


class Phases:
    """wall time of a handler's steps.  Both modes: the re-encode of the touched rows into the
    .porenc (shared code) and the tree step as a whole (tree_s: the full rebuild, or the cache
    update + fold + sidecar + .portree); everything else (raw file write, metadata) is other_s.
    The cached handler's tree step is also split: its mapping of the image and rehash
    (cache_update_s), the fold and tree (cache_tree_s), the copy of the rehashed chunk rows
    (cache_copy_cvs_s), the sidecar write and the .portree write."""

    def __init__(self, fh):
        self.t = {}
        self.top = ("reencode_rows_s", "tree_s")
        for name, key in [("_reencode_rows", "reencode_rows_s"), ("recalculate_merkle_tree", "tree_s"),
                          ("_update_chunk_cache", "tree_s"), ("write_tree", "portree_write_s")]:
            setattr(fh, name, self._wrap(getattr(fh, name), key))
        if fh.chunk_cache is not None:
            for name, key in [("update_file", "cache_update_s"), ("tree", "cache_tree_s"), ("copy_cvs", "cache_copy_cvs_s")]:
                setattr(fh.chunk_cache, name, self._wrap(getattr(fh.chunk_cache, name), key))
            PF.write_chunk_cv_sidecar = self._wrap(PF.write_chunk_cv_sidecar, "sidecar_write_s")

    def _wrap(self, fn, key):
        def run(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t
        return run

    def take(self, total):
        t, self.t = self.t, {}
        t["other_s"] = total - sum(t.get(k, 0.0) for k in self.top)
        return {k: round(v, 5) for k, v in t.items()}


def run_ops(fh, ops, reps, rng, cached, check):
    """{op: {"times_s": [...], ...}}: each op `reps` times, then once more under the profiler"""
    rb = fh.pre_encoded_size * 7
    out = {}
    phases = Phases(fh)
    for name, start_row, n_bytes in ops:
        times, image_bytes, equal, ph, profiled_repeat = [], [], [], [], None
        row_lo = row_hi = lo = hi = 0
        for rep in range(reps + 1):
            profiled = rep == reps
            if profiled:
                lcpc2d.prof_enable(True)
                lcpc2d.prof_reset()
            data = rng.integers(0, 256, n_bytes, dtype=np.uint8).tobytes()
            old_rows = fh.rows_written
            t = time.perf_counter()
            if name.startswith("append"):
                row_lo = fh.total_data_bytes // rb
                tree = fh.append_bytes(data)
                row_hi = fh.rows_written
            else:
                row_lo, row_hi = start_row, -(-(start_row * rb + n_bytes) // rb)
                _, tree = fh.edit_bytes(start_row * rb, data)
            dt = time.perf_counter() - t
            p = phases.take(dt)
            if profiled:
                prof = {k: [round(ms, 4), int(cnt)] for k, (ms, cnt) in lcpc2d.prof_stats().items()}
                lcpc2d.prof_enable(False)
                profiled_repeat = {"total_s": round(dt, 5), "phases": p, "regions_ms_count": prof}
            else:
                times.append(dt)
                ph.append(p)
            if cached:
                lo, hi = PF.ColumnChunkCache.update_chunk_range(old_rows, fh.rows_written, row_lo, row_hi)
                assert (lo, hi) == fh.last_chunk_range
                read_rows = min(fh.rows_written, first_row(hi)) - first_row(lo)
                if check:
                    equal.append(bool(fh.recalculate_tree_only() == tree))
            else:
                read_rows = fh.rows_written
            if not profiled:
                image_bytes.append(read_rows * fh.encoded_size * 8)
        out[name] = {"times_s": [round(x, 5) for x in times],
                     "median_s": round(statistics.median(times), 5) if times else None,
                     "spread_s": round(max(times) - min(times), 5) if times else None, "phases": ph,
                     "image_bytes_read": image_bytes, "rows": row_hi - row_lo, "profiled_repeat": profiled_repeat}
        if cached:
            out[name]["chunks_rehashed"] = hi - lo
            # None: not compared (--no-check)
            out[name]["tree_equals_full_rebuild"] = all(equal) if check else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1 << 30, help="bytes of the stored file (default 1 GiB)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files go (default: a fresh temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_edit_incremental.json"))
    ap.add_argument("--no-check", action="store_true", help="skip the full rebuild after each incremental operation")
    args = ap.parse_args()
    L.set_device(0)
    n = args.size
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(n)
    rb = pre * 7
    work = args.dir or tempfile.mkdtemp(prefix="pos_edit_bench_")
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
        create_s = time.perf_counter() - t
        rows = fh.rows_written
        edit_bytes = min(MIB, max(rb, n // 4))
        mid = (rows // 2) if rows > 1 else 0
        ops = [("edit_one_row", mid, min(rb, n)), ("edit_1MiB", max(0, mid - (edit_bytes // rb) // 2), edit_bytes),
               ("append_1MiB", None, min(MIB, max(rb, n // 4)))]
        res = {"what": "FileHandler edit_bytes / append_bytes on one stored file: full rebuild of the tree from the "
                       "whole .porenc (chunk_cache=False, the parent's behaviour) against the column chunk-CV cache "
                       "(chunk_cache=True); wall times measured, image_bytes_read derived from row and chunk counts",
               "size": n, "pre": pre, "enc": enc, "rows_written": rows, "row_capacity": fh.row_capacity,
               "n_chunks": PF.leaf_n_chunks(rows), "reps": args.reps, "create_s": round(create_s, 3)}
        res["full_rebuild"] = run_ops(fh, ops, args.reps, rng, False, False)
        del fh
        t = time.perf_counter()
        fh = PF.FileHandler.new_attach_to_existing_ulid(files, ULID, chunk_cache=True)
        res["attach_rebuild_s"] = round(time.perf_counter() - t, 4)   # no sidecar yet: one full pass
        t = time.perf_counter()
        again = PF.FileHandler.new_attach_to_existing_ulid(files, ULID, chunk_cache=True)
        res["attach_load_s"] = round(time.perf_counter() - t, 4)      # the sidecar just written
        del again
        res["incremental"] = run_ops(fh, ops, args.reps, rng, True, not args.no_check)
        fh.verify_all_files_agree()
        res["verify_all_files_agree"] = True
        res["sidecar_bytes"] = os.path.getsize(fh.chunk_cv_file_handle)
        verdict = {}
        for name, _, _ in ops:
            a, b = res["full_rebuild"][name], res["incremental"][name]
            if not args.reps:
                continue
            verdict[name] = {"full_rebuild_median_s": a["median_s"], "incremental_median_s": b["median_s"],
                             "full_rebuild_spread_s": a["spread_s"],
                             "speedup": round(a["median_s"] / b["median_s"], 2) if b["median_s"] else None,
                             "image_bytes_ratio": round(a["image_bytes_read"][0] / max(1, b["image_bytes_read"][0]), 1),
                             "beats_by_more_than_spread": a["median_s"] - b["median_s"] > a["spread_s"]}
        res["summary"] = verdict
        flags = [res["incremental"][name]["tree_equals_full_rebuild"] for name, _, _ in ops]
        res["trees_equal"] = None if None in flags else all(flags)   # None: nothing was compared
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"size": n, "trees_equal": res["trees_equal"], "summary": verdict}))
    finally:
        if args.dir is None:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
