"""Commit time per digest (lcpc_digest: BLAKE3, SHA-256, SHA3-256, Keccak-256) at the benchmark
shapes; not the bench.py metric.

Shapes: cfg3 (Ligero, Ft127, 2^24 coefficients, rho = 1/2: a row-major codeword of 2^16 columns) and
cfg4 (Brakedown SdigCode3, seed 0, same size: a column-major codeword).  Per digest and shape:
  commit          LcCommit.commit_device from coefficients resident in HBM, `--reps` timed runs after
                  `--warmup` (the call returns once its stream has drained, so the wall time around it
                  is the device time of the commitment plus its launches); median and spread;
  kernels         the leaf pass and the Merkle pass of one more commit, timed on the device with HIP
                  events around their launches (lcpc_prof_*: regions leaf_chunks / leaf_merge for
                  BLAKE3, leaf_digest for the others, merkle); and, with --rocprof, of one separate
                  `rocprofv3 --kernel-trace --stats` run of this tool (kernel durations by name);
  check           after timing, 64 sampled columns at full size: the leaf digest in the tree is the
                  digest of the opened column, the opened path is the tree's siblings, and walking it
                  with hashlib (tests/digest_ref.py) reaches the commitment's root.
With --digest blake3 only entry points from before the digest feature are used, so the same file
runs on an older checkout (--root) for a before / after comparison; --parity FILE embeds such a
comparison (made by alternating runs of both checkouts) in the profile.  Everything is written to
profiles/digest_commit.json; a summary line is printed.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = {"blake3": 0, "sha256": 1, "sha3-256": 2, "keccak256": 3}
LEAF_REGIONS = ("leaf_chunks", "leaf_merge", "leaf_digest")
KERNEL_GROUPS = {"leaf": ("k_leaf_digest", "k_leaf_chunks", "k_leaf_merge", "k_leaf_fold"), "merkle": ("k_merkle",)}


class HipMem:
    """device buffers through the HIP runtime the library links (no torch: one runtime per process)"""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.L = C.CDLL("libamdhip64.so.7")
        self.L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.L.hipFree.argtypes = [C.c_void_p]

    def to_device(self, a):
        p = self.C.c_void_p()
        if self.L.hipMalloc(self.C.byref(p), a.nbytes) or self.L.hipMemcpy(p, a.ctypes.data, a.nbytes, 1):
            raise RuntimeError("hipMalloc / hipMemcpy failed")
        return p.value

    def free(self, p):
        self.L.hipFree(p)


def make_encoding(L, shape, fid, n, digest):
    enc = L.SdigEncoding.new(fid, n, 0) if shape == "cfg4" else L.LigeroEncoding.new(fid, n)
    if digest:  # (BLAKE3: nothing newer than the digest feature is touched)
        enc.set_digest(digest)
    return enc


def reference_digest(digest):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import digest_ref
    return digest_ref, (lambda msgs: digest_ref.digest_many(digest, msgs))


def check_commit(L, comm, fid, digest, n_samples=64):
    """sampled leaves and paths, and the root, against hashlib at full size"""
    R, many = reference_digest(digest)
    n_cols, hashes, root = comm.get_n_cols(), comm.hashes, comm.get_root()
    np2 = (len(hashes) // 32 + 1) // 2
    idx = sorted({0, n_cols - 1} | {int(i) for i in np.random.default_rng(5).integers(0, n_cols, n_samples - 2)})
    cols = comm.open_columns(idx)
    leaves = many([bytes(32) + R.column_bytes(fid, c.col) for c in cols])
    for i, c, leaf in zip(idx, cols, leaves):
        assert hashes[32 * i:32 * i + 32] == leaf, f"leaf {i} differs from the reference digest"
        lo, n, k, h = 0, np2, i, leaf
        for sib in c.path:
            assert sib == hashes[32 * (lo + (k ^ 1)):32 * (lo + (k ^ 1)) + 32], f"path of column {i}"
            h = many([sib + h if k & 1 else h + sib])[0]
            lo, n, k = lo + n, n // 2, k >> 1
        assert h == root == hashes[-32:], f"the path of column {i} does not reach the root"
    return {"sampled_columns": len(idx), "leaves_paths_root_match_hashlib": True}


def bench_one(L, hip, shape, digest_name, args):
    digest = DIGESTS[digest_name]
    fid, n = L.FT127, 1 << args.log_len
    enc = make_encoding(L, shape, fid, n, digest)
    coeffs = L.field_random(fid, n, 9)
    d = hip.to_device(coeffs)
    try:
        ts = []
        for k in range(args.warmup + args.reps):
            t = time.perf_counter()
            comm = L.LcCommit.commit_device(d, n, enc)
            ts.append((time.perf_counter() - t) * 1e3)
            if k + 1 < args.warmup + args.reps:
                del comm
        ts = ts[args.warmup:]
        res = {"n_rows": comm.get_n_rows(), "n_cols": comm.get_n_cols(), "col_major": shape == "cfg4",
               "commit_ms": {"times": [round(x, 3) for x in ts], "median": round(statistics.median(ts), 3),
                             "spread": round(max(ts) - min(ts), 3)}}
        L.prof_enable(True)
        L.prof_reset()
        c2 = L.LcCommit.commit_device(d, n, enc)
        stats = L.prof_stats()
        L.prof_enable(False)
        del c2
        res["kernels_ms_hip_events"] = {
            "leaf": round(sum(stats[k][0] for k in LEAF_REGIONS if k in stats), 4),
            "merkle": round(stats["merkle"][0], 4) if "merkle" in stats else None,
            "regions": {k: [round(v[0], 4), int(v[1])] for k, v in sorted(stats.items()) if not k.startswith(("host_", "rt_"))}}
        if not args.no_check:
            res["check"] = check_commit(L, comm, fid, digest)
        res["root"] = comm.get_root().hex()
        del comm
        return res
    finally:
        hip.free(d)


def rocprof_kernels(shape, digest_name, args):
    """kernel durations by name from one `rocprofv3 --kernel-trace --stats` run of a single commit"""
    out = tempfile.mkdtemp(prefix="digest_rocprof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
           sys.executable, os.path.abspath(__file__), "--root", args.root, "--child", shape, digest_name,
           "--log-len", str(args.log_len)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode:
        return {"error": f"rocprofv3 exit {r.returncode}: {(r.stderr or r.stdout)[-300:]}"}
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel_stats.csv written"}
    groups = {g: {"ms": 0.0, "calls": 0} for g in KERNEL_GROUPS}
    for row in csv.DictReader(open(files[0])):
        name, total = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
        for g, subs in KERNEL_GROUPS.items():
            if any(s in name for s in subs):
                groups[g]["ms"] = round(groups[g]["ms"] + total / 1e6, 4)
                groups[g]["calls"] += int(float(row.get("Calls", 0) or 0))
    groups["commits_in_run"] = 2  # (one warm-up, one more: halve for one commit)
    return groups


def child(L, hip, shape, digest_name, args):
    fid, n = L.FT127, 1 << args.log_len
    enc = make_encoding(L, shape, fid, n, DIGESTS[digest_name])
    d = hip.to_device(L.field_random(fid, n, 9))
    for _ in range(2):
        L.LcCommit.commit_device(d, n, enc)
    hip.free(d)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--digest", default="all", help="all, or a comma-separated list of " + ", ".join(DIGESTS))
    ap.add_argument("--shapes", default="cfg3,cfg4")
    ap.add_argument("--log-len", type=int, default=24)
    ap.add_argument("--reps", type=int, default=7, help="timed commits (median; at least 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--rocprof", action="store_true", help="also one rocprofv3 --kernel-trace --stats run per case")
    ap.add_argument("--child-timeout", type=int, default=180)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured (default: this one)")
    ap.add_argument("--parity", default=None, help="JSON of a before / after comparison to embed in the profile")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "digest_commit.json"))
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "DIGEST"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.root = os.path.abspath(args.root)
    sys.path.insert(0, args.root)
    import lcpc_proof_of_storage_amd as L
    L.set_device(0)
    hip = HipMem()
    if args.child:
        return child(L, hip, args.child[0], args.child[1], args)
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    names = list(DIGESTS) if args.digest == "all" else args.digest.split(",")
    res = {"what": "commit from device-resident coefficients per digest; Ft127, 2^%d coefficients" % args.log_len,
           "root_dir_is_this_checkout": args.root == HERE, "reps": args.reps, "warmup": args.warmup, "shapes": {}}
    for shape in args.shapes.split(","):
        res["shapes"][shape] = {}
        for name in names:
            r = bench_one(L, hip, shape, name, args)
            if args.rocprof:
                r["kernels_ms_rocprofv3"] = rocprof_kernels(shape, name, args)
            res["shapes"][shape][name] = r
        if "blake3" in res["shapes"][shape]:
            base = res["shapes"][shape]["blake3"]["commit_ms"]["median"]
            for name, r in res["shapes"][shape].items():
                r["commit_vs_blake3"] = round(r["commit_ms"]["median"] / base, 3)
    if args.parity:
        res["unchanged_behaviour"] = json.load(open(args.parity))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({s: {k: [v["commit_ms"]["median"], v["kernels_ms_hip_events"]["leaf"],
                              v["kernels_ms_hip_events"]["merkle"]] for k, v in d.items()}
                      for s, d in res["shapes"].items()}))


if __name__ == "__main__":
    main()
