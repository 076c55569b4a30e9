"""Grouped ingest of small files: a whole fleet encoded, hashed and folded to trees in one call
(lcpc_pos_encode_files_grouped) against one lcpc_pos_encode_file per file, the parent's behaviour, in the
same process; not the bench.py metric.  Writes profiles/pos_group_ingest.json and prints a summary line.

Fleets, each in a child process of its own under a time limit (a failing stage ends the run), all at
the default PoS dims of their file size:
  64kib_x4096, 1mib_x1024   equal-sized files
  16mib_x64                 rows above LCPC_POS_INGEST_MAX_ENC: routed to the single path, the end of the range
  mixed                     2048 x 64 KiB, 256 x 1 MiB and 8 x 16 MiB, shuffled
  e2e                       FileHandler.create_from_unencoded_files against a loop of
                            create_from_unencoded_file over 256 files of 64 KiB on disk
For a fleet: the wall time of the call into in-memory targets with images (row_capacity = rows) and
roots only (no image asked for; the single call has no such form and still returns its tree), and the
device time of the call's launches (the library's HIP-event regions: pos_group_ingest for the grouped
call, every kernel region of the single calls), each the median of --reps (5) after one warm-up, the two
sides alternating; the spread is max - min.  The results are compared byte for byte.  Verdict per figure
(DESIGN §4b): the grouped median plus its spread is below the singles' median.
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
    "64kib_x4096": [(64 * KIB, 4096)],
    "1mib_x1024": [(MIB, 1024)],
    "16mib_x64": [(16 * MIB, 64)],
    "mixed": [(64 * KIB, 2048), (MIB, 256), (16 * MIB, 8)],
}
E2E_FILES, E2E_BYTES = 256, 64 * KIB
LIMIT_S = 420   # per stage
HOST_REGIONS = ("rt_", "pos_group_ingest_gather", "pos_group_ingest_scatter", "cache_", "pos_group_gather")
u8p = C.POINTER(C.c_uint8)


def summary(ts, unit):
    return {f"times_{unit}": [round(x, 5) for x in ts], f"median_{unit}": round(statistics.median(ts), 5),
            f"spread_{unit}": round(max(ts) - min(ts), 5)}


def wall_pair(f, g, reps):
    """f and g alternating; the first run of each warms the pools and is dropped"""
    tf, tg = [], []
    for _ in range(reps + 1):
        for fn, ts in ((f, tf), (g, tg)):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
    return summary(tf[1:], "s"), summary(tg[1:], "s")


def regions_ms(lcpc2d, pick, fn, reps):
    """(device time, regions) of the regions pick(name) accepts per call of fn, after a warm-up"""
    ts, counts, names = [], [], set()
    lcpc2d.prof_enable(True)
    for _ in range(reps + 1):
        lcpc2d.prof_reset()
        fn()
        st = {n: v for n, v in lcpc2d.prof_stats().items() if pick(n)}
        ts.append(sum(v[0] for v in st.values()))
        counts.append(sum(v[1] for v in st.values()))
        names |= set(st)
    lcpc2d.prof_enable(False)
    lcpc2d.prof_reset()
    return summary(ts[1:], "ms") | {"regions": counts[-1], "names": sorted(names)}


def verdict(grouped, singles, unit):
    g, s = grouped[f"median_{unit}"], singles[f"median_{unit}"]
    return {"singles_over_grouped": round(s / g, 2) if g else None,
            "grouped_wins": g + grouped[f"spread_{unit}"] < s}


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
    dims = {int(b): P.get_aspect_ratio_default_from_file_len(int(b))[:2] for b in set(sizes.tolist())}
    pres, encs = [dims[int(b)][0] for b in sizes], [dims[int(b)][1] for b in sizes]
    rows = [-(-(-(-int(b) // 7)) // p) for b, p in zip(sizes, pres)]
    datas = [rng.integers(0, 256, int(b), dtype=np.uint8) for b in sizes]
    img_g = [np.zeros((e, r), np.uint64) for e, r in zip(encs, rows)]
    img_s = [np.zeros((e, r), np.uint64) for e, r in zip(encs, rows)]
    tree_s = [np.zeros((2 * e - 1, 32), np.uint8) for e in encs]
    tiles, groups = P.ingest_plan(sizes, pres, encs)
    enc_bytes = sum(r * e * 8 for r, e in zip(rows, encs))
    tree_bytes = sum((2 * e - 1) * 32 for e in encs)
    res = {"files": {str(b): n for b, n in FLEETS[name]}, "n_jobs": int(n_jobs), "image_bytes": int(sizes.sum()),
           "dims": {str(b): list(d) for b, d in dims.items()},
           "plan": {"groups": int(groups), "tiles": int(tiles.size),
                    "single_path_jobs": int((tiles["launch"] == P.GROUP_SINGLE).sum()),
                    "launches_at_most": int(groups) * P.INGEST_LAUNCHES_PER_GROUP},
           "bytes_moved": {"up": int(sizes.sum()), "back_with_images": int(enc_bytes + tree_bytes),
                           "back_roots_only": int(tree_bytes)}}
    got = {}

    def grouped_images():
        got["img"] = P.encode_files_grouped_into(datas, pres, encs, img_g, rows, True, False, False)

    def grouped_roots():
        got["roots"] = P.commit_roots_of_files(datas, pres, encs)

    def singles(images=True):
        rw = C.c_size_t()
        for j in range(n_jobs):
            d, t = datas[j].ctypes.data_as(u8p), tree_s[j].ctypes.data_as(u8p)
            if images:
                rc = lib.lcpc_pos_encode_file(d, datas[j].size, pres[j], encs[j], rows[j], img_s[j].ctypes.data_as(u8p),
                                              t, C.byref(rw))
                if rc:
                    raise RuntimeError(f"status {rc}: {N.last_error()}")
                continue
            # roots only: the single call's digest-only form is its writer without an image
            h = N.vp()
            assert lib.lcpc_pos_writer_new(pres[j], encs[j], None, 0, 0, C.byref(h)) == 0
            try:
                assert lib.lcpc_pos_writer_push_bytes(h, d, datas[j].size) == 0
                assert lib.lcpc_pos_writer_finalize(h, None, t, None, None) == 0
            finally:
                lib.lcpc_pos_writer_free(h)

    g, s = wall_pair(grouped_images, singles, reps)
    for j in range(n_jobs):
        assert np.array_equal(img_g[j], img_s[j]), f"job {j}: the grouped image differs from the single call's"
        assert np.array_equal(got["img"][j]["tree"], tree_s[j]), f"job {j}: the grouped tree differs"
    res["with_images"] = {"grouped": g, "singles": s, "wall": verdict(g, s, "s")}
    g, s = wall_pair(grouped_roots, lambda: singles(False), reps)
    assert got["roots"] == [t[-1].tobytes() for t in tree_s], "the grouped roots differ from the single calls'"
    res["roots_only"] = {"grouped": g, "singles": s, "wall": verdict(g, s, "s")}
    dg = regions_ms(lcpc2d, lambda n: n == "pos_group_ingest" or (groups == 0 and not n.startswith(HOST_REGIONS)),
                    grouped_images, reps)
    ds = regions_ms(lcpc2d, lambda n: not n.startswith(HOST_REGIONS), singles, reps)
    res["device_time"] = {"grouped": dg, "singles": ds, "verdict": verdict(dg, ds, "ms")}
    print("STAGE_RESULT " + json.dumps(res))


def e2e_stage(reps, seed):
    import shutil
    import tempfile
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import pos as P, pos_files as PF
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    rng = np.random.default_rng(seed)
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(E2E_BYTES)
    blobs = [rng.integers(0, 256, E2E_BYTES, dtype=np.uint8).tobytes() for _ in range(E2E_FILES)]
    names = [f"01BENCH{i:019d}" for i in range(E2E_FILES)]
    with tempfile.TemporaryDirectory() as tmp:
        def fresh(tag):
            d = os.path.join(tmp, tag)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(os.path.join(d, "up"))
            srcs = []
            for n, b in zip(names, blobs):
                srcs.append(os.path.join(d, "up", n + ".bin"))
                with open(srcs[-1], "wb") as f:
                    f.write(b)
            return d, srcs

        def grouped(d, srcs):
            PF.FileHandler.create_from_unencoded_files([(n, s, pre, enc) for n, s in zip(names, srcs)], d)

        def loop(d, srcs):
            for n, s in zip(names, srcs):
                PF.FileHandler.create_from_unencoded_file(n, s, pre, enc, d)

        res = {"files": E2E_FILES, "file_bytes": E2E_BYTES, "pre": pre, "enc": enc}
        tg, tl = [], []
        for _ in range(reps + 1):   # alternating; the first run of each is dropped
            for make, ts in ((grouped, tg), (loop, tl)):
                d, srcs = fresh(make.__name__)
                t = time.perf_counter()
                make(d, srcs)
                ts.append(time.perf_counter() - t)
        res["grouped"], res["loop"] = summary(tg[1:], "s"), summary(tl[1:], "s")
        for n in names:
            for ext in ("porraw", "porenc", "portree", "meta"):
                with open(os.path.join(tmp, "grouped", f"{n}.{ext}"), "rb") as a, \
                        open(os.path.join(tmp, "loop", f"{n}.{ext}"), "rb") as b:
                    assert a.read() == b.read(), (n, ext)
    res["wall"] = verdict(res["grouped"], res["loop"], "s")
    print("STAGE_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", nargs="+", default=list(FLEETS) + ["e2e"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--stage")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_group_ingest.json"))
    a = ap.parse_args()
    if a.stage:
        return e2e_stage(a.reps, a.seed) if a.stage == "e2e" else fleet_stage(a.stage, a.reps, a.seed)
    result = {"tool": "tools/pos_group_ingest_bench.py", "reps": a.reps, "fleets": {}, "not_measured": []}
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
            brief[name] = {"grouped_s": st["grouped"]["median_s"], "loop_s": st["loop"]["median_s"]}
        else:
            brief[name] = {"images_s": [st["with_images"]["grouped"]["median_s"], st["with_images"]["singles"]["median_s"]],
                           "roots_s": [st["roots_only"]["grouped"]["median_s"], st["roots_only"]["singles"]["median_s"]],
                           "device_ms": [st["device_time"]["grouped"]["median_ms"],
                                         st["device_time"]["singles"]["median_ms"]]}
    print(json.dumps(brief | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
