"""Generate tests/golden/pos_group_plans.json: the work lists of the grouped ingest, scrub and repair
planners over fixed fleets of jobs, pinned as hashes.

    python tests/golden/gen_pos_group_plans.py

Host only: lcpc_pos_ingest_plan, lcpc_pos_scrub_plan and lcpc_pos_repair_plan are pure functions of
the jobs' sizes and of LCPC_POS_GROUP_BYTES.  The file was recorded from the library as it stood
before the three planners were folded into one (csrc/pos_rowgroup_plan.hpp) and is not regenerated
when the planner's code moves: tests/test_pos_group_plans_golden.py recomputes every record.  A record
is n_tiles, n_launches and the SHA-256 of the tile array's bytes (lcpc_pos_ingest_tile: job, row_lo,
row_hi as u64, launch, workgroup as u32, little endian); the fleets themselves are pinned by the
SHA-256 of their columns, so a change to this file's fleets cannot pass for a change of the planner.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pos_group_plans.json")

ENCS = tuple(1 << k for k in range(1, 11)) + (2048,)       # every grouped enc, and one for the single path
ROWS = (0, 1, 7, 8, 9, 124, 125, 1023, 1024, 1025)          # leaf_chunks steps between 124 and 125 rows
GROUP_BYTES = (None, 65536, 4096)                           # LCPC_POS_GROUP_BYTES: unset, and lowered twice
MAX_JOBS = 1 << 16                                          # LCPC_POS_INGEST_MAX_JOBS
DATA_BYTES = 7                                              # bytes of a file per stored element


def pres_of(enc):
    """1, enc - 1 and a pre that is no power of two (where enc leaves room for one)"""
    return sorted({1, enc - 1} | ({3 * enc // 4 - 1} if enc >= 8 else set()) | ({3} if enc >= 4 else set()))


def bads_of(pre, enc):
    """no listed column, one, all the code can restore, and one more: a job that does no work"""
    return (0, 1, enc - pre, enc - pre + 1)


def image_bytes(rng, rows, pre):
    """a file of `rows` rows at `pre`: the last row full or ragged"""
    if rows == 0:
        return 0
    return DATA_BYTES * pre * (rows - 1) + int(rng.randint(1, DATA_BYTES * pre + 1))


def fleet(seed, triples):
    """columns of a fleet from (enc, pre, rows, n_bad) with n_bad None: drawn from bads_of"""
    rng = np.random.RandomState(seed)
    enc, pre, rows, bad, nb = [], [], [], [], []
    for e, p, r, b in triples:
        enc.append(e), pre.append(p), rows.append(r)
        bad.append(bads_of(p, e)[rng.randint(4)] if b is None else b)
        nb.append(image_bytes(rng, r, p))
    return {"seed": seed, "n_bytes": nb, "rows": rows, "pre": pre, "enc": enc, "n_bad": bad}


def fleets():
    out = {}
    # every enc x its pres x every row count, enc the slow index: groups of one row length
    out["every_enc_pre_rows"] = fleet(0x5101, [(e, p, r, None) for e in ENCS for p in pres_of(e) for r in ROWS])
    # the same jobs shuffled: row lengths mixed within a group (longest-first order, wg_slots packing)
    rng = np.random.RandomState(0x5102)
    jobs = [(e, p, r, None) for e in ENCS for p in pres_of(e) for r in ROWS]
    out["every_enc_pre_rows_shuffled"] = fleet(0x5103, [jobs[i] for i in rng.permutation(len(jobs))])
    # many short files of mixed dims, drawn
    rng = np.random.RandomState(0x5104)
    mixed = []
    for _ in range(3000):
        e = int(rng.choice(ENCS))
        mixed.append((e, int(rng.choice(pres_of(e))), int(rng.choice((0, 1, 2, 7, 8, 9, 17, 124, 125))), None))
    out["mixed_short"] = fleet(0x5105, mixed)
    # more one-row jobs than a group takes
    out["one_row_jobs"] = fleet(0x5106, [(2, 1, 1, 0)] * (MAX_JOBS + 100))
    # repair: jobs that do no work (X) at the start, in the middle and at the end of a group, and between
    # groups.  At 4096 bytes a group holds four jobs of 8 rows of 16 points (w) or one of 32 rows.
    w, X, big = (16, 8, 8, 1), (16, 8, 8, 9), (16, 8, 32, 8)
    out["repair_no_work_placed"] = fleet(0x5107, [X, w, w, w, w, w, X, w, w, X, w, w, w, w, X, X, X, big, X, big, w, w,
                                                  w, X, X])
    # repair: a fleet of such jobs only, of mixed dims (one that would go single by its enc among them)
    out["repair_no_work_only"] = fleet(0x5108, [(e, p, r, e - p + 1) for e in (2, 16, 1024, 2048)
                                                for p in (1, e - 1) for r in (0, 9)])
    return out


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fleet_sha(f) -> str:
    return sha(np.array([f[k] for k in ("n_bytes", "rows", "pre", "enc", "n_bad")], dtype="<u8"))


def records(pos, f):
    """one record per entry for the fleet f under the LCPC_POS_GROUP_BYTES now in the environment"""
    out = {}
    for name, args in (("ingest_plan", (f["n_bytes"], f["pre"], f["enc"])),
                       ("scrub_plan", (f["rows"], f["pre"], f["enc"])),
                       ("repair_plan", (f["rows"], f["pre"], f["enc"], f["n_bad"]))):
        tiles, launches = getattr(pos, name)(*args)
        out[name] = {"n_tiles": int(tiles.size), "n_launches": int(launches), "tiles_sha256": sha(tiles)}
    return out


def group_bytes_key(gb) -> str:
    return "default" if gb is None else str(gb)


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from lcpc_proof_of_storage_amd import pos
    saved = os.environ.pop("LCPC_POS_GROUP_BYTES", None)
    out = {}
    try:
        for name, f in fleets().items():
            rec = {"seed": f["seed"], "n_jobs": len(f["enc"]), "fleet_sha256": fleet_sha(f), "plans": {}}
            for gb in GROUP_BYTES:
                if gb is None:
                    os.environ.pop("LCPC_POS_GROUP_BYTES", None)
                else:
                    os.environ["LCPC_POS_GROUP_BYTES"] = str(gb)
                rec["plans"][group_bytes_key(gb)] = records(pos, f)
            out[name] = rec
    finally:
        os.environ.pop("LCPC_POS_GROUP_BYTES", None)
        if saved is not None:
            os.environ["LCPC_POS_GROUP_BYTES"] = saved
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
