"""CPU: the host-only side of the grouped stored-file audit -- lcpc_pos_group_plan's
work list, the argument checks of the two grouped entries, and lcpc_field_to_montgomery against
Python integers.  No device is needed; with one the valid calls simply succeed."""
import ctypes as C

import numpy as np
import pytest

INVALID_ARG, NO_DEVICE, UNSUPPORTED = 30, 33, 34
PRES = (8, 16, 64, 256, 16384)
ROWS = (1, 7, 8, 9, 17, 513)
CUTS = (0, 1, 6, 7, 55, 56, 57)
WAVE, WG_WAVES, MAX_WORKGROUPS = 64, 4, 1 << 24   # k_left_mul_bytes' launcher refuses 2^24 workgroups


@pytest.fixture(scope="module")
def pos():
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


def file_rows(n_bytes, pre):
    return -(-(-(-n_bytes // 7)) // pre)


def random_fleet(rng, n_jobs, pres=PRES, rows=ROWS):
    """(sizes, pres): n_bytes = rows 7 pre - k, at least one byte"""
    p = rng.choice(pres, n_jobs)
    r = rng.choice(rows, n_jobs)
    k = rng.choice(CUTS, n_jobs)
    return np.maximum(r * 7 * p - k, 1).astype(np.int64), p.astype(np.int64)


def check_plan(pos, sizes, pres, group_bytes=None):
    """every property the work list promises; returns (tiles, n_launches)"""
    group_bytes = group_bytes or pos.GROUP_STAGE_BYTES
    sizes, pres = np.asarray(sizes, np.int64), np.asarray(pres, np.int64)
    tiles, n_launches = pos.left_multiply_group_plan(sizes, pres)
    job = tiles["job"].astype(np.int64)
    assert job.min() == 0 and job.max() == sizes.size - 1 and np.all(tiles["row_lo"] < tiles["row_hi"])
    rows = np.array([file_rows(int(n), int(p)) for n, p in zip(sizes, pres)], np.int64)
    runs = -(-pres // 8)
    # exactly-once cover: per job the row intervals partition [0, rows), and within a row interval the
    # run intervals partition [0, runs); a record names one job, so no tile crosses a job
    order = np.lexsort((tiles["run_lo"], tiles["row_lo"], job))
    t, j = tiles[order], job[order]
    same_band = (j[1:] == j[:-1]) & (t["row_lo"][1:] == t["row_lo"][:-1])
    assert np.all(t["row_hi"][1:][same_band] == t["row_hi"][:-1][same_band])
    assert np.all(t["run_lo"][1:][same_band] == t["run_hi"][:-1][same_band])
    band_start = np.concatenate([[True], ~same_band])
    band_end = np.concatenate([~same_band, [True]])
    assert np.all(t["run_lo"][band_start] == 0)
    assert np.all(t["run_hi"][band_end] == runs[j[band_end]])
    b_job, b_lo, b_hi = j[band_start], t["row_lo"][band_start].astype(np.int64), t["row_hi"][band_start].astype(np.int64)
    same_job = b_job[1:] == b_job[:-1]
    assert np.all(b_lo[1:][same_job] == b_hi[:-1][same_job])
    job_start = np.concatenate([[True], ~same_job])
    job_end = np.concatenate([~same_job, [True]])
    assert np.all(b_lo[job_start] == 0) and np.all(b_hi[job_end] == rows[b_job[job_end]])
    assert np.array_equal(np.unique(b_job), np.arange(sizes.size))
    # routing: exactly the jobs the grouped kernel cannot take, one record each
    single = tiles["launch"] == pos.GROUP_SINGLE
    want_single = ((pres < 8) | (pres & (pres - 1) != 0) | (sizes > group_bytes))
    assert np.array_equal(np.sort(job[single]), np.flatnonzero(want_single))
    g = tiles[~single]
    assert n_launches == (int(g["launch"].max()) + 1 if g.size else 0)
    if not g.size:
        return tiles, n_launches
    gj = g["job"].astype(np.int64)
    width = (g["run_hi"] - g["run_lo"]).astype(np.int64)
    depth = (g["row_hi"] - g["row_lo"]).astype(np.int64)
    assert np.all(width == np.minimum(runs[gj], WAVE))
    # at least 8 rows per thread where a job has them: only a job's last split may be shallower
    assert np.all((depth >= 8) | (g["row_hi"].astype(np.int64) == rows[gj]))
    # a wave: one row count, one width, at most 64 lanes
    key = g["launch"].astype(np.int64) << 32 | g["wave"].astype(np.int64)
    o = np.argsort(key, kind="stable")
    ks, first = np.unique(key[o], return_index=True)
    for arr in (depth[o], width[o]):
        assert np.array_equal(np.maximum.reduceat(arr, first), np.minimum.reduceat(arr, first))
    assert np.all(np.add.reduceat(width[o], first) <= WAVE)
    # a launch: waves numbered from 0 without gaps, a grid below the single kernel's limit, consecutive
    # jobs whose 8-byte aligned images fit the staging group
    prev_hi = -1
    for launch in range(n_launches):
        m = g["launch"] == launch
        waves = np.unique(g["wave"][m])
        assert np.array_equal(waves, np.arange(waves.size))
        assert -(-waves.size // WG_WAVES) < MAX_WORKGROUPS
        jobs = np.unique(gj[m])
        assert jobs[0] > prev_hi and np.array_equal(jobs, np.arange(jobs[0], jobs[-1] + 1))
        assert not want_single[jobs[0]:jobs[-1] + 1].any()
        assert int(((sizes[jobs] + 7) & ~7).sum()) <= group_bytes or jobs.size == 1
        prev_hi = jobs[-1]
    return tiles, n_launches


@pytest.mark.parametrize("n_jobs", [1, 2, 3, 257, 5000])
def test_random_fleets_are_covered_exactly_once(pos, n_jobs):
    rng = np.random.default_rng(n_jobs)
    for trial in range(3 if n_jobs <= 257 else 1):
        # (a fleet of 5000 with many 16384-wide files would be all table: keep those rare there)
        pres = PRES if n_jobs <= 257 else (8, 8, 16, 16, 64, 64, 256, 256, 256, 16384)
        sizes, p = random_fleet(rng, n_jobs, pres)
        check_plan(pos, sizes, p)


@pytest.mark.parametrize("pre", PRES)
@pytest.mark.parametrize("rows", ROWS)
def test_uniform_fleets(pos, pre, rows):
    """every (pre, rows) alone, as three equal jobs and with every ragged tail"""
    n = rows * 7 * pre
    check_plan(pos, [n], [pre])
    check_plan(pos, [n] * 3, [pre] * 3)
    check_plan(pos, [max(n - k, 1) for k in CUTS], [pre] * len(CUTS))


def test_adversarial_fleets(pos):
    check_plan(pos, [1] * 5000, [8] * 5000)                        # 5000 one-byte files
    tiles, launches = check_plan(pos, [56] * 5000, [8] * 5000)     # 5000 one-row files: 64 jobs per wave
    assert launches == 1 and np.unique(tiles["wave"]).size == -(-5000 // 64)
    check_plan(pos, [7 * 16384 * 17] * 257, [16384] * 257)         # wide jobs: many workgroups each
    check_plan(pos, [7 * 16384 * 513] * 2, [16384] * 2)            # above the staging group: single path
    alt = [(56, 8) if i % 2 else (7 * 16384 * 9, 16384) for i in range(257)]
    check_plan(pos, [a for a, _ in alt], [b for _, b in alt])
    # jobs that fill a group to the byte, and one byte more
    half = pos.GROUP_STAGE_BYTES // 2
    _, launches = check_plan(pos, [half, half, 56], [256, 256, 8])
    assert launches == 2
    _, launches = check_plan(pos, [half, half - 56, 56], [256, 256, 8])
    assert launches == 1


def test_split_rule(pos):
    """left_mul_split's rule for the launch as a whole: ceil(2^18 / the launch's runs) ways at the
    most, and never below 8 rows per thread.  (A staging group of 32 MiB holds fewer than 2^18 threads
    of 8 rows, so inside one the floor decides.)"""
    tiles, _ = pos.left_multiply_group_plan([7 * 8 * 17, 7 * 8 * 8, 7 * 8 * 3], [8, 8, 8])
    t0 = np.sort(tiles[tiles["job"] == 0], order="row_lo")
    assert [(int(a), int(b)) for a, b in zip(t0["row_lo"], t0["row_hi"])] == [(0, 8), (8, 16), (16, 17)]
    assert (tiles["job"] == 1).sum() == 1 and (tiles["job"] == 2).sum() == 1
    # pre = 16384 with 9 rows: two splits, 32 workgroup-wide tiles each
    tiles, _ = pos.left_multiply_group_plan([7 * 16384 * 9], [16384])
    assert tiles.size == 2 * (16384 // 8 // WAVE) and np.unique(tiles["wave"]).size == tiles.size
    # a launch of many jobs: the same floor for each
    tiles, launches = check_plan(pos, [7 * 512 * 293] * 31, [512] * 31)
    assert launches == 1
    for j in (0, 30):
        tj = tiles[tiles["job"] == j]
        assert tj.size == -(-293 // 8) and int((tj["row_hi"] - tj["row_lo"]).max()) == 8


def test_routing_of_other_widths_and_large_files(pos):
    big = pos.GROUP_STAGE_BYTES + 7 * 256
    sizes, pres = [560, 7 * 24 * 5, 560, big, 560], [8, 24, 16, 256, 8]
    tiles, launches = check_plan(pos, sizes, pres)
    for j in (1, 3):
        rec = tiles[tiles["job"] == j]
        assert rec.size == 1 and rec["launch"][0] == pos.GROUP_SINGLE and rec["wave"][0] == 0
        assert (rec["row_lo"][0], rec["row_hi"][0]) == (0, file_rows(sizes[j], pres[j]))
        assert (rec["run_lo"][0], rec["run_hi"][0]) == (0, -(-pres[j] // 8))
    # a routed job ends the group before it
    assert launches == 3
    assert [int(tiles[tiles["job"] == j]["launch"][0]) for j in (0, 2, 4)] == [0, 1, 2]


def test_plan_is_a_pure_function(pos, monkeypatch):
    rng = np.random.default_rng(5)
    sizes, pres = random_fleet(rng, 257)
    a, la = pos.left_multiply_group_plan(sizes, pres)
    pos.left_multiply_group_plan(sizes[::-1].copy(), pres[::-1].copy())
    b, lb = pos.left_multiply_group_plan(sizes.copy(), pres.copy())
    assert la == lb and a.tobytes() == b.tobytes()
    # the staging seam can only lower the group size; lower, the same jobs make more launches
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 40))
    c, lc = pos.left_multiply_group_plan(sizes, pres)
    assert lc == la and c.tobytes() == a.tobytes()
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    _, small = check_plan(pos, sizes, pres, group_bytes=1 << 20)
    assert small > la


def test_plan_arguments(native):
    lib = native.load()
    n, launches = C.c_size_t(), C.c_size_t()
    nb, pr = (C.c_size_t * 2)(56, 56), (C.c_size_t * 2)(8, 8)
    buf = (native.PosGroupTile * 1)()
    assert lib.lcpc_pos_group_plan(nb, pr, 2, None, 0, C.byref(n), C.byref(launches)) == 0
    assert (n.value, launches.value) == (2, 1)
    assert lib.lcpc_pos_group_plan(nb, pr, 2, buf, 1, C.byref(n), None) == 0 and n.value == 2   # cap < needed
    assert lib.lcpc_pos_group_plan(nb, pr, 2, None, 0, None, None) == 0
    assert lib.lcpc_pos_group_plan(None, pr, 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert lib.lcpc_pos_group_plan(nb, None, 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert lib.lcpc_pos_group_plan(nb, pr, 2, None, 1, C.byref(n), None) == INVALID_ARG
    assert lib.lcpc_pos_group_plan(nb, pr, 0, None, 0, C.byref(n), None) == INVALID_ARG
    assert lib.lcpc_pos_group_plan((C.c_size_t * 2)(56, 0), pr, 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert lib.lcpc_pos_group_plan(nb, (C.c_size_t * 2)(0, 8), 2, None, 0, C.byref(n), None) == INVALID_ARG


def test_grouped_entries_refuse_before_the_device(native):
    """Both entries check their arguments before they ask for a device, so the refusals carry
    LCPC_ERR_INVALID_ARG with or without one; valid arguments reach the device (LCPC_ERR_NO_DEVICE
    here, success on a GPU machine)."""
    from lcpc_proof_of_storage_amd import lcpc2d
    lib = native.load()
    have_device = lcpc2d.device_count() > 0
    images = [np.full(56 * 2, 3, np.uint8), np.full(100, 5, np.uint8)]
    sizes, pres = [112, 100], [8, 16]
    rows = [file_rows(n, p) for n, p in zip(sizes, pres)]
    lefts, out = np.ones(sum(rows), np.uint64), np.zeros(sum(pres), np.uint64)
    u64p = native.u64p
    ok = dict(bytes=(C.c_void_p * 2)(*[a.ctypes.data for a in images]), n_bytes=(C.c_size_t * 2)(*sizes),
              pre=(C.c_size_t * 2)(*pres), n_jobs=2, lefts=lefts.ctypes.data_as(u64p), n_left=lefts.size,
              out=out.ctypes.data_as(u64p), n_out=out.size)

    def host(**kw):
        a = {**ok, **kw}
        return lib.lcpc_pos_left_multiply_bytes_grouped(a["bytes"], a["n_bytes"], a["pre"], a["n_jobs"], a["lefts"],
                                                        a["n_left"], a["out"], a["n_out"])

    def device(arena=4096, offsets=(0, 112), **kw):
        a = {**ok, **kw}
        of = (C.c_size_t * 2)(*offsets) if offsets is not None else None
        return lib.lcpc_pos_left_multiply_bytes_grouped_device(arena, of, a["n_bytes"], a["pre"], a["n_jobs"],
                                                               a["lefts"], a["n_left"], a["out"], a["n_out"])

    for call in (host, device):
        for name in ("n_bytes", "pre", "lefts", "out"):
            assert call(**{name: None}) == INVALID_ARG, (call.__name__, name)
        assert call(n_jobs=0) == INVALID_ARG
        assert call(n_bytes=(C.c_size_t * 2)(112, 0)) == INVALID_ARG        # an empty job
        assert call(pre=(C.c_size_t * 2)(8, 0)) == INVALID_ARG
        assert call(n_left=lefts.size - 1) == INVALID_ARG and call(n_left=lefts.size + 1) == INVALID_ARG
        assert call(n_out=out.size - 1) == INVALID_ARG and call(n_out=out.size + 1) == INVALID_ARG
        assert call(pre=(C.c_size_t * 2)(8, 8)) == INVALID_ARG              # totals of other dims
    assert host(bytes=None) == INVALID_ARG
    assert host(bytes=(C.c_void_p * 2)(images[0].ctypes.data, None)) == INVALID_ARG
    assert device(arena=None) == INVALID_ARG and device(offsets=None) == INVALID_ARG
    assert device(offsets=(0, 116)) == INVALID_ARG and device(offsets=(1, 112)) == INVALID_ARG
    assert device(arena=4100) == INVALID_ARG
    assert host() == (0 if have_device else NO_DEVICE)
    if not have_device:   # (with a device the arena above is no device memory: not called)
        assert device() == NO_DEVICE


def test_field_to_montgomery_against_python_integers(pos, native):
    p = pos.FT63_MODULUS
    rng = np.random.default_rng(63)
    edge = [0, 1, p - 1, p, p + 1, 2**63, 2**64 - 1, 2**56 - 1]
    v = np.concatenate([np.array(edge, np.uint64), rng.integers(0, 2**64, 4096, dtype=np.uint64)])
    got = pos.field_to_montgomery(v)
    assert got.dtype == np.uint64 and got.shape == v.shape
    assert [int(x) for x in got] == [(int(x) << 64) % p for x in v]
    assert pos.field_to_montgomery(v.reshape(-1, 8)).shape == (v.size // 8, 8)
    assert pos.field_to_montgomery(np.zeros(0, np.uint64)).size == 0
    lib = native.load()
    w = v.copy()   # in place
    assert lib.lcpc_field_to_montgomery(0, w.ctypes.data_as(native.u64p), w.ctypes.data_as(native.u64p), w.size) == 0
    assert np.array_equal(w, got)
    assert lib.lcpc_field_to_montgomery(1, w.ctypes.data_as(native.u64p), w.ctypes.data_as(native.u64p), 1) == UNSUPPORTED
    assert lib.lcpc_field_to_montgomery(5, w.ctypes.data_as(native.u64p), w.ctypes.data_as(native.u64p), 1) == INVALID_ARG
    assert lib.lcpc_field_to_montgomery(0, None, w.ctypes.data_as(native.u64p), 1) == INVALID_ARG
    assert lib.lcpc_field_to_montgomery(0, None, None, 0) == 0
