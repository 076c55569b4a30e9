"""The client's check of a whole fleet of stored-file audit responses in one call
(pos.client_verify_evaluations_grouped -> lcpc_pos_verify_evaluations_grouped) against a loop of
pos.client_verify_evaluation over the same responses, the parent's behaviour, in the same process; not
the bench.py metric.  Writes profiles/pos_group_verify.json and prints a summary line.

Fleets, each in a child process of its own under a time limit (a failing stage ends the run), all at
the default PoS dims of their file size with the soundness column count get_PoS_soudness_n_cols(pre, enc):
  64kib_x1024, 1mib_x256, 16mib_x16   equal-sized files
  mixed                                512 x 64 KiB, 64 x 1 MiB and 4 x 16 MiB, shuffled
The responses are honest ones built in memory (random elements committed, the columns opened, u^T Enc(M)
for the point's left vector); a fleet has DISTINCT_FILES distinct files per size, every job its own
point and columns: what the check costs does not depend on which file a response is about.
For a fleet: the wall time of both from host memory, the device time (the sum of the library's
HIP-event regions during the call; host phases and runtime calls that share the table are left out by
name and the whole table is kept beside the sum), each the median of --reps (5) after one warm-up, the
spread max - min; and the bytes each side uploads per job, computed from the sizes its entries upload.
Verdicts and values are compared word for word.  Verdict per figure: the grouped median
plus its spread is below the singles' median.  --headline records bench.py result lines handed over
as JSON files (parent and this tree).
"""
import argparse
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
    "64kib_x1024": [(64 * KIB, 1024)],
    "1mib_x256": [(MIB, 256)],
    "16mib_x16": [(16 * MIB, 16)],
    "mixed": [(64 * KIB, 512), (MIB, 64), (16 * MIB, 4)],
}
DISTINCT_FILES = 4
LIMIT_S = 420   # per stage
HOST_REGIONS = ("pos_group_verify_call", "pos_group_verify_gather", "cache_image_read", "pos_group_gather")


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


def device_ms(lcpc2d, fn, reps):
    """the sum of the device regions per call of fn, after a warm-up, and the last call's table"""
    ts, table = [], {}
    lcpc2d.prof_enable(True)
    for _ in range(reps + 1):
        lcpc2d.prof_reset()
        fn()
        table = {n: v for n, v in lcpc2d.prof_stats().items() if v[1]}
        ts.append(sum(ms for n, (ms, _) in table.items() if not n.startswith("rt_") and n not in HOST_REGIONS))
    lcpc2d.prof_enable(False)
    lcpc2d.prof_reset()
    return summary(ts[1:], "ms") | {"regions": {n: [round(ms, 4), int(c)] for n, (ms, c) in sorted(table.items())}}


def verdict(grouped, singles, unit):
    g, s = grouped[f"median_{unit}"], singles[f"median_{unit}"]
    return {"singles_over_grouped": round(s / g, 2) if g else None,
            "grouped_wins": g + grouped[f"spread_{unit}"] < s}


def upload_bytes(n_rows, pre, enc, n_cols):
    """(grouped, singles) bytes uploaded for one job"""
    plen = enc.bit_length() - 1
    cols, stride = n_cols * n_rows * 8, n_cols * 4 * ((2 * n_rows + 3) & ~3)
    paths = n_cols * plen * 32
    grouped = stride + paths + 32 + 16 * n_cols + 8 * n_rows + 64 + 2 * enc * 8
    singles = (cols                                            # lcpc_hash_field_columns
               + 32 * n_cols + paths + 8 * n_cols + 32         # lcpc_verify_leaf_paths
               + 8                                             # lcpc_pos_side_vectors
               + enc * 8                                       # lcpc_ifft_oi_rows
               + 2 * pre * 8                                   # the dot
               + enc * 8                                       # lcpc_encode
               + cols + 8 * n_rows + enc * 8 + 8 * n_cols)     # lcpc_verify_column_values
    return grouped, singles


def fleet_stage(name, reps, seed):
    import lcpc_proof_of_storage_amd as L
    from lcpc_proof_of_storage_amd import lcpc2d, pos as P
    assert L.device_count() > 0, "this measurement needs a HIP device"
    L.set_device(0)
    rng = np.random.default_rng(seed)
    sizes = np.concatenate([np.full(n, b, np.int64) for b, n in FLEETS[name]])
    rng.shuffle(sizes)
    n_jobs = sizes.size
    points = L.field_random(0, n_jobs, seed)
    commits, audits, up_g, up_s = {}, [], 0, 0
    for j, b in enumerate(sizes.tolist()):
        pre, enc = P.get_aspect_ratio_default_from_file_len(b)[:2]
        n_elems = -(-b // 7)
        n_rows = -(-n_elems // pre)
        key = (b, j % DISTINCT_FILES)
        if key not in commits:
            code = L.LigeroEncoding.new_from_dims(0, pre, enc)
            commits[key] = L.LcCommit.commit(L.field_random(0, n_elems, seed + 7 * len(commits)), code)
        comm = commits[key]
        n_open = min(P.get_PoS_soudness_n_cols(pre, enc), enc)
        cols = sorted(rng.choice(enc, size=n_open, replace=False).tolist())
        left, _ = P.form_side_vectors_for_polynomial_evaluation_from_point(points[j:j + 1], n_rows, pre)
        audits.append((comm.get_root(), 7 * n_elems, pre, enc, points[j:j + 1], cols,
                       P.verifiable_polynomial_evaluation(comm, left), comm.open_columns(cols)))
        g, s = upload_bytes(n_rows, pre, enc, n_open)
        up_g, up_s = up_g + g, up_s + s
    del commits
    tiles, launches = P.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    res = {"files": {str(b): n for b, n in FLEETS[name]}, "n_jobs": int(n_jobs),
           "dims": sorted({(a[2], a[3], len(a[5])) for a in audits}),
           "column_bytes": int(sum(np.asarray(c.col).nbytes for a in audits for c in a[7])),
           "plan": {"launches": int(launches), "records": int(tiles.size),
                    "single_path_jobs": len(set(tiles["job"][tiles["launch"] == P.GROUP_SINGLE].tolist()))},
           "upload_bytes_per_job": {"grouped": round(up_g / n_jobs), "singles": round(up_s / n_jobs)}}
    got, want = [], []

    def grouped():
        got[:] = P.client_verify_evaluations_grouped(audits)

    def singles():
        want[:] = [P.client_verify_evaluation(*a) for a in audits]

    res["grouped"], res["singles"] = wall(grouped, reps), wall(singles, reps)
    assert len(got) == len(want) == n_jobs
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.shape == w.shape and np.array_equal(g, w), "the grouped check differs"
    res["wall"] = verdict(res["grouped"], res["singles"], "s")
    res["grouped_device_time"] = device_ms(lcpc2d, grouped, reps)
    res["singles_device_time"] = device_ms(lcpc2d, singles, reps)
    res["device_time"] = verdict(res["grouped_device_time"], res["singles_device_time"], "ms")
    # the library call inside the grouped wall time (a host region of the last profiled call): the rest is
    # the Python entry's marshalling of the column objects
    res["grouped_library_call_ms"] = res["grouped_device_time"]["regions"].get("pos_group_verify_call", [None])[0]
    print("STAGE_RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleets", nargs="+", default=list(FLEETS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--stage")
    ap.add_argument("--headline", nargs="*", default=[], metavar="LABEL=FILE",
                    help="bench.py result lines to record, e.g. parent_ligero=parent.json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pos_group_verify.json"))
    a = ap.parse_args()
    if a.stage:
        return fleet_stage(a.stage, a.reps, a.seed)
    result = {"tool": "tools/pos_group_verify_bench.py", "reps": a.reps, "distinct_files_per_size": DISTINCT_FILES,
              "fleets": {}, "headline": {}, "not_measured": []}
    for item in a.headline:
        label, path = item.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        result["headline"][label] = json.loads(lines[-1]) if lines else None
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
    brief = {name: {"wall_s": [st["grouped"]["median_s"], st["singles"]["median_s"]],
                    "device_ms": [st["grouped_device_time"]["median_ms"], st["singles_device_time"]["median_ms"]],
                    "upload_per_job": [st["upload_bytes_per_job"]["grouped"], st["upload_bytes_per_job"]["singles"]]}
             for name, st in result["fleets"].items()}
    print(json.dumps(brief | {"not_measured": result["not_measured"]}))
    return 1 if result["not_measured"] else 0


if __name__ == "__main__":
    sys.exit(main())
