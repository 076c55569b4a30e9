"""CPU: the host-only side of the grouped repair of stored files -- lcpc_pos_repair_plan's
work list and the argument checks of lcpc_pos_repair_files_grouped.  No device is needed; with one the
valid call simply succeeds."""
import ctypes as C

import numpy as np
import pytest

INVALID_ARG, FFT_TOO_BIG, NO_DEVICE = 30, 21, 33
ENCS = (2, 4, 16, 32, 256, 1024, 2048)
ROWS = (0, 1, 7, 8, 9, 129)
WG_ELEMS, MAX_WORKGROUPS = 2048, 1 << 24
MAX_JOBS, MAX_ROWS, MAX_TILES, MAX_TREE_BYTES = 1 << 16, 1 << 23, 1 << 20, 64 << 20


@pytest.fixture(scope="module")
def pos():
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


def pres_of(enc):
    return sorted({1, max(enc // 2, 1), enc - 1} | ({24} if enc == 32 else set()))


def bads_of(pre, enc):
    """the erasure counts of the issue: none, one, all the code can restore, one more"""
    return sorted({0, 1, enc - pre, enc - pre + 1})


def random_fleet(rng, n_jobs, encs=ENCS, rows=ROWS):
    e = rng.choice(encs, n_jobs)
    p = np.array([rng.choice(pres_of(int(x))) for x in e])
    r = rng.choice(rows, n_jobs)
    b = np.array([rng.choice(bads_of(int(pp), int(x))) for pp, x in zip(p, e)])
    return r.astype(np.int64), p.astype(np.int64), e.astype(np.int64), b.astype(np.int64)


def check_plan(pos, rows, pres, encs, bads, group_bytes=None):
    """every property the work list promises; returns (tiles, n_groups)"""
    group_bytes = group_bytes or pos.GROUP_STAGE_BYTES
    rows, pres, encs, bads = (np.asarray(a, np.int64) for a in (rows, pres, encs, bads))
    tiles, n_groups = pos.repair_plan(rows, pres, encs, bads)
    again, n_again = pos.repair_plan(rows.copy(), pres.copy(), encs.copy(), bads.copy())
    assert n_again == n_groups and again.tobytes() == tiles.tobytes()          # a pure function
    works = bads <= encs - pres        # the others do no device work: no record, and they end no group
    job = tiles["job"].astype(np.int64)
    lo, hi = tiles["row_lo"].astype(np.int64), tiles["row_hi"].astype(np.int64)
    assert np.all(lo < hi)
    # every (job, row) of a job that does device work in exactly one record: per job the row intervals
    # partition [0, rows)
    order = np.lexsort((lo, job))
    j, a, b = job[order], lo[order], hi[order]
    same = j[1:] == j[:-1]
    assert np.all(a[1:][same] == b[:-1][same])
    first, last = np.concatenate([[True], ~same]), np.concatenate([~same, [True]])
    if j.size:
        assert np.all(a[first] == 0) and np.all(b[last] == rows[j[last]])
    assert np.array_equal(np.unique(job), np.flatnonzero((rows > 0) & works))
    # routing: enc above the grouped kernel's rows, or an image (rows rounded up to even) above a group
    packed = ((rows + 1) & ~1) * encs * 8
    want_single = works & ((encs > pos.REPAIR_MAX_ENC) | (packed > group_bytes))
    single = tiles["launch"] == pos.GROUP_SINGLE
    assert np.array_equal(np.sort(job[single]), np.flatnonzero(want_single & (rows > 0)))
    assert np.all(tiles["workgroup"][single] == 0) and np.all(lo[single] == 0) and np.all(hi[single] == rows[job[single]])
    g = tiles[~single]
    gj = g["job"].astype(np.int64)
    depth = (g["row_hi"] - g["row_lo"]).astype(np.int64)
    assert np.all(depth <= pos.REPAIR_TILE_ROWS)
    assert np.all((depth == pos.REPAIR_TILE_ROWS) | (g["row_hi"].astype(np.int64) == rows[gj]))
    assert pos.REPAIR_LAUNCHES_PER_GROUP == 4
    if g.size:
        assert int(g["launch"].max()) < n_groups
    prev_hi = -1
    for launch in np.unique(g["launch"]):
        m = g["launch"] == launch
        jobs = np.unique(gj[m])
        assert jobs[0] > prev_hi
        span = np.arange(jobs[0], jobs[-1] + 1)
        assert not want_single[span].any()
        span = span[works[span]]
        if span.size > 1:
            assert int(packed[span].sum()) <= group_bytes
            assert span.size <= MAX_JOBS and int(rows[span].sum()) <= MAX_ROWS and int(m.sum()) <= MAX_TILES
            assert int(((2 * encs[span] - 1) * 32).sum()) <= MAX_TREE_BYTES
        # workgroups numbered from 0 without gaps; the tiles of one share enc and fit its LDS slots
        wg = g["workgroup"][m].astype(np.int64)
        ids = np.unique(wg)
        assert np.array_equal(ids, np.arange(ids.size)) and ids.size < MAX_WORKGROUPS
        e = encs[gj[m]]
        o = np.argsort(wg, kind="stable")
        _, start, count = np.unique(wg[o], return_index=True, return_counts=True)
        assert np.array_equal(np.maximum.reduceat(e[o], start), np.minimum.reduceat(e[o], start))
        slots = np.maximum(1, WG_ELEMS // (pos.REPAIR_TILE_ROWS * e[o][start]))
        assert np.all(count <= slots)
        prev_hi = jobs[-1]
    return tiles, n_groups


@pytest.mark.parametrize("n_jobs", [1, 2, 3, 257, 5000])
def test_random_fleets_are_covered_exactly_once(pos, n_jobs):
    rng = np.random.default_rng(n_jobs)
    for trial in range(3 if n_jobs <= 257 else 1):
        check_plan(pos, *random_fleet(rng, n_jobs))


@pytest.mark.parametrize("enc", ENCS)
def test_uniform_fleets(pos, enc):
    for pre in pres_of(enc):
        if pre >= enc:
            continue
        for nb in bads_of(pre, enc):
            check_plan(pos, list(ROWS), [pre] * len(ROWS), [enc] * len(ROWS), [nb] * len(ROWS))
            for rows in ROWS:
                check_plan(pos, [rows], [pre], [enc], [nb])


def test_tiles_and_workgroups(pos):
    tiles, groups = check_plan(pos, [17, 8, 0, 3], [8] * 4, [16] * 4, [1, 0, 8, 8])
    assert groups == 1
    t0 = np.sort(tiles[tiles["job"] == 0], order="row_lo")
    assert [(int(a), int(b)) for a, b in zip(t0["row_lo"], t0["row_hi"])] == [(0, 8), (8, 16), (16, 17)]
    assert (tiles["job"] == 1).sum() == 1 and (tiles["job"] == 2).sum() == 0 and (tiles["job"] == 3).sum() == 1
    # 1000 one-row files at 16 / 8: one group, 16 tiles to a workgroup, whatever their erasure sets
    tiles, groups = check_plan(pos, [1] * 1000, [8] * 1000, [16] * 1000, [k % 9 for k in range(1000)])
    assert groups == 1 and tiles.size == 1000 and np.unique(tiles["workgroup"]).size == -(-1000 // 16)
    # rows of 256 points and more: a tile has a workgroup to itself
    tiles, _ = check_plan(pos, [74] * 3, [128] * 3, [256] * 3, [1, 16, 128])
    assert np.unique(tiles["workgroup"]).size == tiles.size == 3 * -(-74 // 8)
    # mixed lengths in one group
    _, groups = check_plan(pos, [100, 30, 20, 1, 0, 2], [1, 24, 512, 15, 8, 255], [2, 32, 1024, 16, 16, 256],
                           [1, 8, 512, 0, 3, 1])
    assert groups == 1
    # only files of zero rows: a group with no tile
    tiles, groups = check_plan(pos, [0, 0], [8, 1], [16, 2], [8, 0])
    assert tiles.size == 0 and groups == 1


def test_jobs_beyond_the_code_do_no_work(pos):
    # more listed columns than enc - pre: no record, no launch of their own, and the group goes on past them
    tiles, groups = check_plan(pos, [9, 9, 9], [8] * 3, [16] * 3, [1, 9, 8])
    assert groups == 1 and set(tiles["job"]) == {0, 2}
    tiles, groups = check_plan(pos, [9, 9], [8, 1], [16, 2], [9, 2])
    assert groups == 0 and tiles.size == 0
    # also where the job would have been routed
    tiles, groups = check_plan(pos, [9, 9, 9], [8, 1024, 8], [16, 2048, 16], [0, 1025, 0])
    assert groups == 1 and set(tiles["job"]) == {0, 2}


def test_routing(pos):
    gb = pos.GROUP_STAGE_BYTES
    over = gb // (256 * 8) + 2         # rows of 256 points whose image exceeds a group
    rows, pres, encs = [10, 5, 10, over, 10], [8, 1024, 8, 128, 8], [16, 2048, 16, 256, 16]
    tiles, groups = check_plan(pos, rows, pres, encs, [1, 3, 8, 1, 0])
    for j in (1, 3):
        rec = tiles[tiles["job"] == j]
        assert rec.size == 1 and rec["launch"][0] == pos.GROUP_SINGLE
    # a routed job ends the group before it
    assert groups == 3
    assert [int(tiles[tiles["job"] == j]["launch"][0]) for j in (0, 2, 4)] == [0, 1, 2]
    # a routed file of zero rows has no record and still splits the groups
    tiles, groups = check_plan(pos, [1, 0, 1], [8, 1024, 8], [16, 2048, 16], [1, 1, 1])
    assert groups == 2 and tiles.size == 2
    # jobs that fill a group to the byte, and one more
    half = gb // 2 // (256 * 8)
    _, groups = check_plan(pos, [half, half, 2], [128, 128, 8], [256, 256, 16], [1, 128, 0])
    assert groups == 2
    _, groups = check_plan(pos, [half, half - 2, 2], [128, 128, 8], [256, 256, 16], [1, 128, 0])
    assert groups == 1


def test_the_seam_only_lowers_the_group(pos, monkeypatch):
    rng = np.random.default_rng(5)
    fleet = random_fleet(rng, 2000, encs=(256, 1024), rows=(8, 9, 129))
    a, ga = pos.repair_plan(*fleet)
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 40))
    c, gc = pos.repair_plan(*fleet)
    assert gc == ga and c.tobytes() == a.tobytes()
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    _, small = check_plan(pos, *fleet, group_bytes=1 << 20)
    assert small > ga
    for n_jobs in (1, 2, 3, 257):
        check_plan(pos, *random_fleet(rng, n_jobs), group_bytes=1 << 20)
    # a job above the lowered group goes the single way, in the middle of the queue
    tiles, groups = check_plan(pos, [10, 514, 10], [8, 128, 8], [16, 256, 16], [1, 1, 1], group_bytes=1 << 20)
    assert groups == 2 and tiles[tiles["job"] == 1]["launch"][0] == pos.GROUP_SINGLE


def test_plan_arguments(pos, native):
    lib = native.load()
    sz2 = C.c_size_t * 2
    rw, pr, en, nb = sz2(1, 1), sz2(8, 8), sz2(16, 16), sz2(1, 8)
    buf = (native.PosIngestTile * 1)()
    plan = lib.lcpc_pos_repair_plan

    def refused(*args):
        """an argument error, with the outputs as they were"""
        n, launches = C.c_size_t(77), C.c_size_t(77)
        buf[0].job = 77
        st = plan(*args, C.byref(n), C.byref(launches))
        assert (n.value, launches.value, buf[0].job) == (77, 77, 77)
        return st

    n, launches = C.c_size_t(), C.c_size_t()
    assert plan(rw, pr, en, nb, 2, None, 0, C.byref(n), C.byref(launches)) == 0
    assert (n.value, launches.value) == (2, 1)
    assert plan(rw, pr, en, nb, 2, buf, 1, C.byref(n), None) == 0 and n.value == 2   # cap < needed
    assert plan(rw, pr, en, nb, 2, None, 0, None, None) == 0
    assert refused(None, pr, en, nb, 2, buf, 1) == INVALID_ARG
    assert refused(rw, None, en, nb, 2, buf, 1) == INVALID_ARG
    assert refused(rw, pr, None, nb, 2, buf, 1) == INVALID_ARG
    assert refused(rw, pr, en, None, 2, buf, 1) == INVALID_ARG
    assert refused(rw, pr, en, nb, 2, None, 1) == INVALID_ARG
    assert refused(rw, pr, en, nb, 0, buf, 1) == INVALID_ARG
    assert refused(rw, sz2(8, 0), en, nb, 2, buf, 1) == INVALID_ARG
    assert refused(rw, pr, sz2(16, 24), nb, 2, buf, 1) == INVALID_ARG   # no power of two
    assert refused(rw, pr, sz2(16, 8), nb, 2, buf, 1) == INVALID_ARG    # enc <= pre
    big = 1 << (two_adicity(pos.FT63_MODULUS) + 1)
    assert refused(rw, pr, sz2(16, big), nb, 2, buf, 1) == FFT_TOO_BIG
    assert plan(sz2(1, 0), pr, en, nb, 2, None, 0, C.byref(n), None) == 0 and n.value == 1  # an empty file is legal
    assert plan(rw, pr, en, sz2(9, 8), 2, None, 0, C.byref(n), None) == 0 and n.value == 1  # too many listed: legal
    with pytest.raises(ValueError):
        pos.repair_plan([1, 2], [8], [16, 16], [0, 0])


def two_adicity(p):
    return ((p - 1) & -(p - 1)).bit_length() - 1


def test_grouped_entry_refuses_before_the_device(pos, native):
    """The entry checks its arguments before it asks for a device and before it writes a byte, so the
    refusals carry their own status with or without one; valid arguments reach the device
    (LCPC_ERR_NO_DEVICE here, success on a GPU machine)."""
    from lcpc_proof_of_storage_amd import lcpc2d
    lib = native.load()
    have_device = lcpc2d.device_count() > 0
    dims, rows = [(8, 16), (24, 32)], [9, 5]
    porenc = [np.zeros(e * (r + 1) * 8, np.uint8) for r, (_, e) in zip(rows, dims)]
    bad = [np.array([3, 0], np.uint64), np.array([31, 7], np.uint64)]
    leaves = [np.zeros(e * 32, np.uint8) for _, e in dims]
    outs = [[np.full(2 * r * 8, 0xA5, np.uint8), np.full(2 * 32, 0xA5, np.uint8),
             np.full((2 * e - 1) * 32, 0xA5, np.uint8), np.full(32, 0xA5, np.uint8)] for r, (_, e) in zip(rows, dims)]

    def call(n_jobs=2, null=False, **kw):
        jobs = []
        for j in range(2):
            f = dict(porenc=porenc[j].ctypes.data, pre=dims[j][0], enc=dims[j][1], rows_written=rows[j],
                     row_capacity=rows[j] + 1, bad_cols=bad[j].ctypes.data, n_bad=2, leaves=leaves[j].ctypes.data,
                     cols_out=outs[j][0].ctypes.data, digests_out=outs[j][1].ctypes.data,
                     tree_out=outs[j][2].ctypes.data, root_out=outs[j][3].ctypes.data, status=77)
            if j == 1:
                f.update(kw)
            jobs.append(native.PosRepairJob(**f))
        arr = (native.PosRepairJob * 2)(*jobs)
        st = lib.lcpc_pos_repair_files_grouped(None if null else arr, n_jobs)
        if st != 0:
            assert all(a.status == 77 for a in arr)
            for o in outs:
                for a in o:
                    assert np.all(a == 0xA5)
        return st

    assert call(null=True) == INVALID_ARG
    assert call(n_jobs=0) == INVALID_ARG
    assert call(porenc=None) == INVALID_ARG                    # no image, rows > 0
    assert call(rows_written=rows[1] + 2) == INVALID_ARG       # rows_written > row_capacity
    assert call(pre=0) == INVALID_ARG
    assert call(enc=24) == INVALID_ARG                         # enc <= pre
    assert call(enc=48) == INVALID_ARG                         # no power of two
    assert call(enc=0) == INVALID_ARG and call(enc=1, pre=1) == INVALID_ARG
    assert call(bad_cols=None) == INVALID_ARG                  # a count without a list
    assert call(bad_cols=np.array([5, 32], np.uint64).ctypes.data) == INVALID_ARG   # an index >= enc
    assert call(bad_cols=np.array([5, 5], np.uint64).ctypes.data) == INVALID_ARG    # a duplicate
    assert call(leaves=None) == INVALID_ARG                    # a tree without leaves
    assert call(leaves=None, tree_out=None) == INVALID_ARG     # a root without leaves
    big = 1 << (two_adicity(pos.FT63_MODULUS) + 1)
    assert call(enc=big, leaves=None, tree_out=None, root_out=None) == FFT_TOO_BIG
    if not have_device:
        assert call() == NO_DEVICE
        assert call(porenc=None, rows_written=0, row_capacity=0) == NO_DEVICE      # an empty file is legal
        assert call(leaves=None, tree_out=None, root_out=None, cols_out=None, digests_out=None) == NO_DEVICE
        assert call(bad_cols=None, n_bad=0) == NO_DEVICE                            # the consistency check alone
        nine = np.arange(9, dtype=np.uint64)
        assert call(bad_cols=nine.ctypes.data, n_bad=9) == NO_DEVICE                # more than enc - pre: a verdict
    with pytest.raises(ValueError):
        pos.repair_files_grouped([None], [8], [16, 16], [0], [0], [[]])
