"""No device: the work list of the grouped check of audit responses (lcpc_pos_verify_group_plan,
csrc/pos_verify_group_host.cpp) and the argument errors of
lcpc_pos_verify_evaluations_grouped, which come before any device work."""
import ctypes as C

import numpy as np
import pytest

from lcpc_proof_of_storage_amd import _native as N
from lcpc_proof_of_storage_amd import pos

# the row counts at which a column's leaf goes from 1 to 2, ..., 5 to 6 chunks, and where the first
# block is exactly full
ROWS = (1, 3, 4, 5, 124, 125, 252, 253, 380, 381, 508, 509, 637)
N_COLS = (0, 1, 63, 64, 65, 309)
GROUP_BYTES = 32 << 20
INVALID_ARG, NO_DEVICE = 30, 33


def rows_of(file_len, pre):
    return -(-(-(-file_len // 7)) // pre)


def chunks_of(rows):
    return -(-(8 + 2 * rows) // 256)


def col_bytes(rows):
    return 4 * ((2 * rows + 3) & ~3)


def make(n_jobs, seed):
    rng = np.random.default_rng(seed)
    pres = rng.choice([8, 16, 24, 64], size=n_jobs)
    rows = rng.choice(ROWS, size=n_jobs)
    lens = [int(7 * (r * p - rng.integers(0, p)) - rng.integers(0, 7)) for r, p in zip(rows, pres)]
    return lens, [int(p) for p in pres], [int(c) for c in rng.choice(N_COLS, size=n_jobs)]


def check_plan(lens, pres, ncs, group_bytes=GROUP_BYTES):
    tiles, launches = pos.verify_group_plan(lens, pres, ncs)
    # every (job, column, chunk) exactly once
    want = sum(nc * chunks_of(rows_of(n, p)) for n, p, nc in zip(lens, pres, ncs))
    seen = set()
    for t in tiles:
        for c in range(int(t["col_lo"]), int(t["col_hi"])):
            key = (int(t["job"]), c, int(t["chunk"]))
            assert key not in seen
            seen.add(key)
    assert len(seen) == want
    for j, c, k in seen:
        assert c < ncs[j] and k < chunks_of(rows_of(lens[j], pres[j]))
    grouped = tiles[tiles["launch"] != pos.GROUP_SINGLE]
    # a record is one wave: one job, one chunk, at most 64 columns; the waves of a launch count from 0
    assert ((grouped["col_hi"] - grouped["col_lo"]) <= 64).all() and (grouped["col_hi"] > grouped["col_lo"]).all()
    assert sorted(set(grouped["launch"].tolist())) == list(range(launches))
    for n in range(launches):
        g = grouped[grouped["launch"] == n]
        assert g["wave"].tolist() == list(range(len(g)))
        assert (len(g) + 3) // 4 < 1 << 24
        jobs = sorted(set(g["job"].tolist()))
        # consecutive jobs (those without columns leave no record) that fit the group
        between = range(jobs[0], jobs[-1] + 1)
        assert all(j in jobs or ncs[j] == 0 for j in between)
        assert sum(ncs[j] * col_bytes(rows_of(lens[j], pres[j])) for j in jobs) <= group_bytes or len(jobs) == 1
        assert sum(ncs[j] for j in jobs) <= 1 << 16
    single = tiles[tiles["launch"] == pos.GROUP_SINGLE]
    for j in set(single["job"].tolist()):
        assert ncs[j] * col_bytes(rows_of(lens[j], pres[j])) > group_bytes or ncs[j] > 1 << 16 or \
            rows_of(lens[j], pres[j]) > group_bytes // 8
    # launches are in job order
    firsts = [int(grouped["job"][grouped["launch"] == n].min()) for n in range(launches)]
    assert firsts == sorted(firsts)
    return tiles, launches


@pytest.mark.parametrize("n_jobs", [1, 2, 257, 3000])
def test_plan_invariants(n_jobs, monkeypatch):
    monkeypatch.delenv("LCPC_POS_GROUP_BYTES", raising=False)
    lens, pres, ncs = make(n_jobs, n_jobs)
    tiles, launches = check_plan(lens, pres, ncs)
    again, again_launches = pos.verify_group_plan(lens, pres, ncs)
    assert again_launches == launches and np.array_equal(again, tiles)   # a pure function
    assert not (tiles["launch"] == pos.GROUP_SINGLE).any()
    # lowering the seam only adds launches (and routes what no longer fits to the single sequence)
    last = launches
    for gb in (1 << 20, 1 << 16, 1 << 13):
        monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(gb))
        _, n = check_plan(lens, pres, ncs, gb)
        singles = len(set(pos.verify_group_plan(lens, pres, ncs)[0]["job"][
            pos.verify_group_plan(lens, pres, ncs)[0]["launch"] == pos.GROUP_SINGLE].tolist()))
        assert n + singles >= last
        last = n + singles
    # raising it does nothing
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 40))
    assert pos.verify_group_plan(lens, pres, ncs)[1] == launches


def test_every_boundary_row_count_and_column_count(monkeypatch):
    monkeypatch.delenv("LCPC_POS_GROUP_BYTES", raising=False)
    lens, pres, ncs = [], [], []
    for r in ROWS:
        for nc in N_COLS:
            lens.append(7 * 8 * r), pres.append(8), ncs.append(nc)
    tiles, launches = check_plan(lens, pres, ncs)
    assert launches == 1
    for j, (r, nc) in enumerate((r, nc) for r in ROWS for nc in N_COLS):
        assert (tiles["job"] == j).sum() == -(-nc // 64) * chunks_of(r)
    assert [chunks_of(r) for r in ROWS] == [1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6] and chunks_of(636) == 5


def test_a_job_above_the_group_goes_single(monkeypatch):
    monkeypatch.delenv("LCPC_POS_GROUP_BYTES", raising=False)
    big_rows = GROUP_BYTES // 8 // 309 + 1          # 309 columns of these rows exceed 32 MiB
    lens, pres, ncs = [7 * 8 * 5, 7 * 64 * big_rows, 7 * 8 * 125], [8, 64, 8], [3, 309, 16]
    tiles, launches = check_plan(lens, pres, ncs)
    assert launches == 2
    single = tiles[tiles["launch"] == pos.GROUP_SINGLE]
    assert set(single["job"].tolist()) == {1} and len(single) == chunks_of(big_rows)
    assert (single["col_lo"] == 0).all() and (single["col_hi"] == 309).all()
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", "4096")
    tiles, launches = check_plan(lens, pres, ncs, 4096)
    assert set(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE].tolist()) == {1, 2} and launches == 1


def test_plan_argument_errors():
    L = N.load()
    sz = (C.c_size_t * 2)
    n = C.c_size_t()
    ok = (sz(56, 56), sz(8, 8), sz(1, 1))
    assert L.lcpc_pos_verify_group_plan(*ok, 2, None, 0, C.byref(n), None) == 0 and n.value == 2
    assert L.lcpc_pos_verify_group_plan(*ok, 0, None, 0, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(None, ok[1], ok[2], 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(ok[0], None, ok[2], 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(ok[0], ok[1], None, 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(*ok, 2, None, 5, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(sz(56, 0), ok[1], ok[2], 2, None, 0, C.byref(n), None) == INVALID_ARG
    assert L.lcpc_pos_verify_group_plan(ok[0], sz(0, 8), ok[2], 2, None, 0, C.byref(n), None) == INVALID_ARG
    with pytest.raises(ValueError):
        pos.verify_group_plan([56], [8, 8], [1])


class Job:
    """one well-formed lcpc_pos_audit_job (its arrays kept alive) and the means to spoil a field"""

    def __init__(self, **changes):
        self.root = np.zeros(32, np.uint8)
        self.idx = np.array(changes.pop("idx_values", [1, 5, 9]), np.uint64)
        self.cols = np.zeros((3, 2), np.uint64)
        self.paths = np.zeros(3 * 4 * 32, np.uint8)
        self.result = np.zeros(16, np.uint64)
        f = dict(root=self.root.ctypes.data, file_len=7 * 8 * 2, pre=8, enc=16, point=3, idx=self.idx.ctypes.data,
                 n_cols=3, cols=self.cols.ctypes.data, paths=self.paths.ctypes.data, result=self.result.ctypes.data)
        f.update(changes)
        self.c = N.PosAuditJob(**f)


def verify(jobs, n=None, verdict=True, values=True):
    arr = (N.PosAuditJob * max(len(jobs), 1))(*[j.c for j in jobs])
    v = np.zeros(max(len(jobs), 1), np.uint8)
    w = np.zeros(max(len(jobs), 1), np.uint64)
    return N.load().lcpc_pos_verify_evaluations_grouped(
        arr if jobs else None, len(jobs) if n is None else n, v.ctypes.data_as(N.u8p) if verdict else None,
        w.ctypes.data_as(N.u64p) if values else None)


@pytest.mark.parametrize("changes", [
    dict(root=None), dict(idx=None), dict(cols=None), dict(paths=None), dict(result=None),
    dict(pre=0), dict(enc=0), dict(file_len=0),
    dict(enc=24), dict(enc=8), dict(pre=16),
    dict(idx_values=[1, 1, 9]), dict(idx_values=[5, 1, 9]), dict(idx_values=[1, 5, 16]),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_verify_argument_errors_come_before_the_device(changes):
    """Each is LCPC_ERR_INVALID_ARG although this machine has no device: the check comes first.  A bad
    job after a good one is found as well.  (enc = 8 and pre = 16 are enc <= pre; a stored file may
    have any power of two above pre, e.g. 24 / 32.)"""
    bad = Job(**changes)
    assert verify([bad]) == INVALID_ARG
    assert verify([Job(), bad]) == INVALID_ARG


def test_verify_null_arrays_and_no_jobs():
    assert verify([]) == INVALID_ARG
    assert verify([Job()], n=0) == INVALID_ARG
    assert verify([Job()], verdict=False) == INVALID_ARG
    assert verify([Job()], values=False) == INVALID_ARG


def test_verify_without_a_device_is_no_device():
    import lcpc_proof_of_storage_amd as L
    if L.device_count() > 0:
        pytest.skip("a device is present: the argument checks above are what runs here")
    assert verify([Job()]) == NO_DEVICE
    assert verify([Job(n_cols=0, idx=None, cols=None, paths=None)]) == NO_DEVICE   # no openings is allowed
    with pytest.raises(L.DeviceError):
        pos.client_verify_evaluations_grouped([(bytes(32), 7 * 8 * 2, 8, 16, np.array([3], np.uint64), [], np.zeros(16, np.uint64), [])])
    with pytest.raises(ValueError):
        pos.client_verify_evaluations_grouped([(bytes(32), 7 * 8 * 2, 8, 16, np.array([3], np.uint64), [2, 1], np.zeros(16, np.uint64), [])])
