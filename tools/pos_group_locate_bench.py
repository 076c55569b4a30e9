"""Grouped locate of stored files: the damaged columns of a whole fleet named by the files' own rows in one
call (lcpc_pos_locate_files_grouped) against the per-file loop over the entry that existed before it
(lcpc_pos_locate_porenc; FileHandler.repair(locate=True) on disk), in the same process; not the bench.py
metric.  Writes profiles/pos_group_locate.json and prints a summary line.

Fleets, each in a child process of its own under a time limit (a failing stage ends the run), all at the
default PoS dims of their file size, images with row_capacity = 2 rows as the writer leaves them:
  64kib_x4096_*, 1mib_x1024_*, 16mib_x64_*   (the 16 MiB files have enc = 4096: routed whole), each with
    _flip   1 % of the files hold one flipped element;
    _run16  every file holds a run of 16 columns overwritten with 0xFF words.  The loop finds them as the
            parent's code path does (lcpc_pos_locate_porenc with no known columns: a pass, a scan, a second
            pass); the grouped call gets them as known columns, as repair_files passes what the
            grouped scrub already named (status 3 there is status 2 of the loop);
    _half   every file holds t = (enc - pre) / 2 wrong elements in one row;
  e2e       pos_files.repair_files(locate=True) against a loop of FileHandler.repair(locate=True) over 256
            files of 64 KiB on disk with every `.portree` deleted and one damaged column each (damaged
            again, outside the clock, before every run).
For a fleet: the wall time of the call and the device time of its launches (the library's HIP-event regions:
pos_group_locate for the grouped call, every kernel region of the single calls), each the median of --reps
(5) after one warm-up, the two sides alternating; the spread is max - min.  The answers of the two sides are
compared with each other and with what was injected.  Verdict per figure: the grouped median plus
its spread is below the singles' median (a routed fleet: within the singles' spread).
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
SIZES = {"64kib_x4096": (64 * KIB, 4096), "1mib_x1024": (MIB, 1024), "16mib_x64": (16 * MIB, 64)}
KINDS = ("flip", "run16", "half")
FLEETS = [f"{s}_{k}" for s in SIZES for k in KINDS]
E2E_FILES, E2E_BYTES = 256, 64 * KIB
LIMIT_S = 420   # per stage
HOST_REGIONS = ("rt_", "pos_group_locate_gather", "pos_group_locate_scatter", "pos_group_repair_gather",
                "pos_group_repair_scatter", "pos_group_scrub_gather", "pos_group_scrub_scatter",
                "pos_group_ingest_gather", "pos_group_ingest_scatter", "cache_", "pos_group_gather")
u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def summary(ts, unit):
    return {f"times_{unit}": [round(x, 5) for x in ts], f"median_{unit}": round(statistics.median(ts), 5),
            f"spread_{unit}": round(max(ts) - min(ts), 5)}


def wall_pair(f, g, reps, before=lambda: None):
    """f and g alternating, before() outside the clock ahead of each; the first run of each warms the pools
    and is dropped"""
    tf, tg = [], []
    for _ in range(reps + 1):
        for fn, ts in ((f, tf), (g, tg)):
            before()
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
            "grouped_wins": g + grouped[f"spread_{unit}"] < s,
            "within_singles_spread": abs(g - s) <= singles[f"spread_{unit}"]}


def fleet_stage(name, reps, seed):
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos as P
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    lib = N.load()
    rng = np.random.default_rng(seed)
    size, kind = name.rsplit("_", 1)
    n_bytes, n_jobs = SIZES[size]
    pre, enc = P.get_aspect_ratio_default_from_file_len(n_bytes)[:2]
    rows = -(-(-(-n_bytes // 7)) // pre)
    cap = 2 * rows
    prime = int(P.FT63_MODULUS)
    datas = [rng.integers(0, 256, n_bytes, dtype=np.uint8) for _ in range(n_jobs)]
    imgs = [np.zeros((enc, cap), np.uint64) for _ in range(n_jobs)]
    P.encode_files_grouped_into(datas, [pre] * n_jobs, [enc] * n_jobs, imgs, [cap] * n_jobs, True, False, False)
    del datas
    knowns, want = [], []
    for j in range(n_jobs):
        cs = np.zeros(enc, np.uint8)
        kn = np.zeros(0, np.uint64)
        if kind == "flip" and j % 100 == 0:
            c, r = (7 * j) % enc, j % rows
            imgs[j][c, r] = np.uint64((int(imgs[j][c, r]) + 1) % prime)
            cs[c] = 1
        elif kind == "run16":
            lo = (7 * j) % (enc - 16 + 1)
            imgs[j][lo:lo + 16, :] = np.uint64(0xFFFFFFFFFFFFFFFF)
            kn = np.arange(lo, lo + 16, dtype=np.uint64)
            cs[lo:lo + 16] = 2
        elif kind == "half":
            t, r = (enc - pre) // 2, j % rows
            cols = rng.permutation(enc)[:t]
            for k, c in enumerate(cols):
                imgs[j][c, r] = np.uint64((int(imgs[j][c, r]) + 1 + k) % prime)
            cs[cols] = 1
        knowns.append(kn)
        want.append(cs)
    tiles, groups = P.repair_plan([rows] * n_jobs, [pre] * n_jobs, [enc] * n_jobs, [k.size for k in knowns])
    res = {"file_bytes": n_bytes, "n_jobs": n_jobs, "pre": pre, "enc": enc, "rows": rows, "row_capacity": cap,
           "damage": kind,
           "plan": {"groups": int(groups), "tiles": int(tiles.size),
                    "single_path_jobs": int((tiles["launch"] == P.GROUP_SINGLE).sum()),
                    "launches_per_group_at_most": P.LOCATE_LAUNCHES_PER_GROUP}}
    got = {}
    args = (imgs, [pre] * n_jobs, [enc] * n_jobs, [rows] * n_jobs, [cap] * n_jobs, knowns)

    def grouped():
        got["g"] = P.locate_files_grouped(*args)

    single = [None] * n_jobs

    def singles():
        for j in range(n_jobs):
            cs = np.zeros(enc, np.uint8)
            nb, nd, nu = C.c_size_t(), C.c_size_t(), C.c_size_t()
            rc = lib.lcpc_pos_locate_porenc(imgs[j].ctypes.data_as(u8p), pre, enc, rows, cap, None, 0,
                                            cs.ctypes.data_as(u8p), C.byref(nb), C.byref(nd), C.byref(nu))
            if rc:
                raise RuntimeError(f"status {rc}: {N.last_error()}")
            single[j] = (cs, nd.value, nu.value)

    g, s = wall_pair(grouped, singles, reps)
    for j in range(n_jobs):
        o = got["g"][j]
        assert o["status"] == 0, j
        cs = o["col_status"].copy()
        cs[cs == 3] = 2
        assert np.array_equal(cs, single[j][0]), f"job {j}: the grouped answer differs"
        assert (o["n_dirty_rows"], o["n_unlocatable_rows"]) == single[j][1:], f"job {j}: the counters differ"
        assert np.array_equal(cs, want[j]) and o["n_unlocatable_rows"] == 0, f"job {j}: not what was injected"
    res["wall"] = {"grouped": g, "singles": s, "verdict": verdict(g, s, "s")}
    res["per_file_us"] = {"grouped": round(1e6 * g["median_s"] / n_jobs, 2), "singles": round(1e6 * s["median_s"] / n_jobs, 2)}
    dg = regions_ms(lcpc2d, lambda n: n == "pos_group_locate" or (groups == 0 and not n.startswith(HOST_REGIONS)),
                    grouped, reps)
    ds = regions_ms(lcpc2d, lambda n: not n.startswith(HOST_REGIONS), singles, reps)
    res["device_time"] = {"grouped": dg, "singles": ds, "verdict": verdict(dg, ds, "ms")}
    res["regions_per_group"] = {"regions_per_call": dg["regions"], "groups": int(groups),
                                "launches_at_most": P.LOCATE_LAUNCHES_PER_GROUP}
    print("STAGE_RESULT " + json.dumps(res))


def e2e_stage(reps, seed):
    import dataclasses
    import tempfile
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import pos as P, pos_files as PF
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    rng = np.random.default_rng(seed)
    pre, enc, _ = P.get_aspect_ratio_default_from_file_len(E2E_BYTES)
    names = [f"01BENCH{i:019d}" for i in range(E2E_FILES)]
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "up"))
        specs = []
        for n in names:
            src = os.path.join(tmp, "up", n + ".bin")
            with open(src, "wb") as f:
                f.write(rng.integers(0, 256, E2E_BYTES, dtype=np.uint8).tobytes())
            specs.append((n, src, pre, enc))
        handlers = PF.FileHandler.create_from_unencoded_files(specs, os.path.join(tmp, "store"))
        roots = [h.get_commit_root() for h in handlers]
        got = {}

        def damage():
            for i, h in enumerate(handlers):
                if os.path.exists(h.merkle_tree_file_handle):
                    os.remove(h.merkle_tree_file_handle)
                with open(h.encoded_file_handle, "r+b") as f:
                    f.seek(((i % enc) * h.row_capacity + i % h.rows_written) * 8)
                    b = f.read(1)
                    f.seek(-1, os.SEEK_CUR)
                    f.write(bytes([b[0] ^ 1]))

        def grouped():
            got["g"] = PF.repair_files(handlers, roots, locate=True)

        def loop():
            got["l"] = [h.repair(expected_root=r, locate=True) for h, r in zip(handlers, roots)]

        g, s = wall_pair(grouped, loop, reps, before=damage)
        assert [dataclasses.asdict(r) for r in got["g"]] == [dataclasses.asdict(r) for r in got["l"]]
        assert all(r.repaired_from == "located+columns+tree" and r.located_columns == [i % enc] for i, r in enumerate(got["g"]))
        assert all(r.clean for r in PF.scrub_files(handlers, roots))
    res = {"files": E2E_FILES, "file_bytes": E2E_BYTES, "pre": pre, "enc": enc, "grouped": g, "loop": s,
           "wall": verdict(g, s, "s")}
    print("STAGE_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", nargs="+", default=FLEETS + ["e2e"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--stage")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_group_locate.json"))
    a = ap.parse_args()
    if a.stage:
        return e2e_stage(a.reps, a.seed) if a.stage == "e2e" else fleet_stage(a.stage, a.reps, a.seed)
    result = {"tool": "tools/pos_group_locate_bench.py", "reps": a.reps, "fleets": {}, "not_measured": []}
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
            brief[name] = {"wall_s": [st["wall"]["grouped"]["median_s"], st["wall"]["singles"]["median_s"]],
                           "device_ms": [st["device_time"]["grouped"]["median_ms"],
                                         st["device_time"]["singles"]["median_ms"]]}
    print(json.dumps(brief | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
