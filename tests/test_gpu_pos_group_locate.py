"""GPU: the grouped locate of stored files (lcpc_pos_locate_files_grouped).  Files are made with
lcpc_pos_encode_file into images prefilled with 0xA5 (capacity 2 rows + 3); the test injects the damage.
Every col_status, counter and status is compared with lcpc_pos_locate_porenc on the same image; row_status
and the located set with what was injected wherever the number of wrong elements of a row is within the
radius (2 t <= N = enc - pre - known), and with the Python reference (rs_locate_ref.py) on the short rows
and on the longest recurrence -- never with the grouped call itself.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import rs_locate_ref as R

pytestmark = pytest.mark.gpu
REGION = "pos_group_locate"
FILL = 0xA5
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
UNRECOVERABLE = 36
ROWS = (0, 1, 7, 8, 9, 125)
DIMS = [(p, 1 << le) for le in range(1, 11) for p in sorted({1, max((1 << le) // 2, 1), (1 << le) - 1})] + \
    [(24, 32), (100, 256)]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


def u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None


class Stored:
    def __init__(self, img, pre, enc, rows, cap):
        self.img, self.pre, self.enc, self.rows, self.cap = img, pre, enc, rows, cap

    def copy(self):
        return Stored(self.img.copy(), self.pre, self.enc, self.rows, self.cap)

    @property
    def elems(self):
        return self.img.view("<u8").reshape(self.enc, self.cap)


_made = {}


def make(native, seed, pre, enc, rows):
    """lcpc_pos_encode_file of a random file of `rows` rows; shared, never changed: tests damage copies"""
    key = (seed, pre, enc, rows)
    if key not in _made:
        lib = native.load()
        data = np.random.default_rng(seed).integers(0, 256, max(rows * 7 * pre - 3, 0), dtype=np.uint8)
        cap = 2 * rows + 3
        img = np.full(enc * cap * 8, FILL, np.uint8)
        tree = np.zeros((2 * enc - 1, 32), np.uint8)
        got = C.c_size_t()
        assert lib.lcpc_pos_encode_file(u8(data), data.size, pre, enc, cap, u8(img), u8(tree), C.byref(got)) == 0
        assert got.value == rows
        _made[key] = Stored(img, pre, enc, rows, cap)
    return _made[key]


def inject(pos, f, per_row):
    """a copy of f with, in row r, the columns per_row[r] holding another canonical element"""
    g = f.copy()
    P = np.uint64(pos.FT63_MODULUS)
    for r, cols in per_row.items():
        for k, c in enumerate(cols):
            v = int(g.elems[c, r])
            g.elems[c, r] = np.uint64((v + 1 + 977 * k + 31 * r) % int(P))
    return g


def wrong_sets(f, known, t, rows, seed):
    """t wrong columns (none of them known) for each of `rows`, a different set per row"""
    free = np.array([c for c in range(f.enc) if c not in set(known)])
    rng = np.random.default_rng(seed)
    t = min(t, free.size)
    return {r: sorted(int(c) for c in rng.permutation(free)[:t]) for r in rows} if t else {}


def expected(f, known, per_row):
    """(row_status, col_status) where every row's wrong elements are within the radius, else None"""
    N = f.enc - f.pre - len(known)
    if any(2 * len(c) > N for c in per_row.values()):
        return None
    rs = np.zeros(f.rows, np.uint8)
    cs = np.zeros(f.enc, np.uint8)
    cs[list(known)] = 3
    for r, cols in per_row.items():
        if cols:
            rs[r] = 1
            cs[cols] = 1
    return rs, cs


def single(native, f, known):
    kb = np.asarray(known, np.uint64)
    cs = np.full(f.enc, 0x5C, np.uint8)
    nb, nd, nu = C.c_size_t(12345), C.c_size_t(12345), C.c_size_t(12345)
    st = native.load().lcpc_pos_locate_porenc(u8(f.img), f.pre, f.enc, f.rows, f.cap,
                                              kb.ctypes.data_as(C.POINTER(C.c_uint64)) if kb.size else None, kb.size,
                                              u8(cs), C.byref(nb), C.byref(nd), C.byref(nu))
    assert st in (0, UNRECOVERABLE)
    return st, cs, nb.value, nd.value, nu.value


def call(pos, files, knowns):
    return pos.locate_files_grouped([f.img for f in files], [f.pre for f in files], [f.enc for f in files],
                                    [f.rows for f in files], [f.cap for f in files], knowns, want_row_status=True)


def check_fleet(pos, native, files, knowns, wants=None, per_file=True):
    res = call(pos, files, knowns)
    assert len(res) == len(files)
    wants = [None] * len(files) if wants is None else wants
    for j, (f, kn, w, r) in enumerate(zip(files, knowns, wants, res)):
        at = (j, f.pre, f.enc, f.rows, len(kn))
        if per_file:
            st, cs, nb, nd, nu = single(native, f, kn)
            assert r["status"] == st, at
            if st:
                assert r["col_status"] is None, at
                continue
            assert np.array_equal(r["col_status"], cs), at
            assert (r["n_bad_cols"], r["n_dirty_rows"], r["n_unlocatable_rows"]) == (nb, nd, nu), at
        if r["status"]:
            continue
        assert r["n_bad_cols"] == int(np.count_nonzero(r["col_status"])), at
        if (r["row_status"] == pos.LOCATE_ROW_NOT_EVALUATED).all() and f.rows:
            continue            # answered by the single-file entry
        assert r["n_dirty_rows"] == int(np.count_nonzero(r["row_status"])), at
        assert r["n_unlocatable_rows"] == int(np.count_nonzero(r["row_status"] == 2)), at
        if w is not None:
            assert r["status"] == 0, at
            assert np.array_equal(r["row_status"], w[0]), at
            assert np.array_equal(r["col_status"], w[1]), at
    return res


def reference(pos, f, known):
    """row_status and the union of the located sets by rs_locate_ref"""
    loc = R.Locator(pos, 0, f.enc, f.pre, known)
    rs, cs = np.zeros(f.rows, np.uint8), np.zeros(f.enc, np.uint8)
    cs[list(known)] = 3
    rows = pos.field_to_montgomery(np.where(f.elems[:, :f.rows] < np.uint64(pos.FT63_MODULUS), f.elems[:, :f.rows], 0))
    for r in range(f.rows):
        st, _, roots = loc.locate(rows[:, r].reshape(f.enc, 1))
        rs[r] = st
        if st == 1:
            cs[roots] = 1
    return rs, cs


def ts_of(N):
    return (0, 1, 2, N // 2, N // 2 + 1)


def test_every_length_row_count_and_error_count(pos, native):
    """every row length at its three pres, the rows cycling through the tile seams, the wrong elements per
    row through 0, 1, 2, the radius and one past it (not locatable, or whatever the per-file entry says)"""
    files, knowns, wants = [], [], []
    for i, (p, e) in enumerate(DIMS):
        for k in range(2):
            o = make(native, 100 + i, p, e, ROWS[(i + k + 1) % len(ROWS)])
            t = ts_of(e - p)[(i + 3 * k) % 5]
            per_row = wrong_sets(o, [], t, range(o.rows), 1000 + 2 * i + k)
            files.append(inject(pos, o, per_row))
            knowns.append([])
            wants.append(expected(o, [], per_row))
    _, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files], [0] * len(files))
    assert groups == 1
    res = check_fleet(pos, native, files, knowns, wants)
    n_ref = 0
    for f, w, r in zip(files, wants, res):
        if w is None:          # one past the radius: a field of 2^63 elements does not miscorrect by chance
            assert (r["row_status"] == 2).all() and not r["col_status"].any()
        if f.enc <= 32:
            rs, cs = reference(pos, f, [])
            assert np.array_equal(r["row_status"], rs) and np.array_equal(r["col_status"], cs)
            n_ref += 1
    assert n_ref >= 25


@pytest.mark.parametrize("t", [63, 64, 65, 127, 128, 129, 256, 257])
def test_cross_lane_and_former_tier_boundaries(pos, native, t):
    o = make(native, 7, 512, 1024, 8)
    per_row = wrong_sets(o, [], t, range(8), t)
    w = expected(o, [], per_row)
    r = check_fleet(pos, native, [inject(pos, o, per_row)], [[]], [w])[0]
    if w is None:
        assert (r["row_status"] == 2).all()


def test_the_longest_recurrence(pos, native):
    """enc = 1024, pre = 1: N = 1023 syndromes, L = 511, the full LDS footprint; and one more wrong element"""
    o = make(native, 8, 1, 1024, 2)
    per_row = wrong_sets(o, [], 511, [0], 1)
    per_row[1] = wrong_sets(o, [], 512, [1], 2)[1]
    f = inject(pos, o, per_row)
    r = check_fleet(pos, native, [f], [[]])[0]
    assert list(r["row_status"]) == [1, 2]
    assert sorted(np.flatnonzero(r["col_status"])) == per_row[0]
    rs, cs = reference(pos, f, [])
    assert np.array_equal(r["row_status"], rs) and np.array_equal(r["col_status"], cs)


def test_rows_of_one_file_differ_and_the_slack_is_not_seen(pos, native):
    files, knowns, wants = [], [], []
    for seed, (p, e, rows) in enumerate([(8, 16, 9), (100, 256, 125), (24, 32, 17), (1, 2, 9)]):
        o = make(native, 300 + seed, p, e, rows)
        t = (e - p) // 2
        per_row = {}
        for r in range(1, rows, 3):                    # a dirty row between clean rows of one tile
            per_row.update(wrong_sets(o, [], 1 + (r % t) if t else 0, [r], 50 * seed + r))
        if t:
            per_row[0] = [0]                           # column 0 and column enc - 1
            per_row[rows - 1] = sorted({0, e - 1})[:t]
        f = inject(pos, o, per_row)
        f.elems[3 % e, rows:] ^= np.uint64(1)          # past rows_written: not the file's
        f.elems[e - 1, rows] = FF
        files.append(f)
        knowns.append([])
        wants.append(expected(o, [], per_row))
    assert all(w is not None for w in wants)
    check_fleet(pos, native, files, knowns, wants)


def test_known_columns(pos, native):
    base = [make(native, 1, 8, 16, 9), make(native, 2, 24, 32, 125), make(native, 3, 100, 256, 9),
            make(native, 5, 512, 1024, 8)]
    files, knowns, wants = [], [], []
    for k, o in enumerate(base):
        room = o.enc - o.pre
        run = list(range(3, 3 + min(room // 2, 16)))
        full = [int(c) for c in np.random.default_rng(k).permutation(o.enc)[:room]]
        for kn in ([], [o.enc - 1], run, full):
            N = room - len(kn)
            for t in sorted({0, N // 2, N // 2 + 1}):    # errors and erasures at 2 t + |E| = enc - pre, and one more
                per_row = wrong_sets(o, kn, t, range(0, o.rows, 2), 7 * k + t)
                f = inject(pos, o, per_row)
                if kn:
                    f.elems[kn, :] = FF                  # what a known column holds cannot matter
                files.append(f)
                knowns.append(kn)
                wants.append(expected(o, kn, per_row) if N else (np.zeros(o.rows, np.uint8), expected(o, kn, {})[1]))
    res = check_fleet(pos, native, files, knowns, wants)
    # a second image that differs only inside the known columns: the same answers, no per-file call
    other = []
    for f, kn in zip(files, knowns):
        g = f.copy()
        if kn:
            g.elems[kn, :] = np.uint64(0x0123456789ABCDEF)
        other.append(g)
    res2 = check_fleet(pos, native, other, knowns, wants, per_file=False)
    for a, b in zip(res, res2):
        assert np.array_equal(a["col_status"], b["col_status"]) and np.array_equal(a["row_status"], b["row_status"])


def test_too_many_known_columns_fail_their_job_alone(pos, native):
    clean = [make(native, 1, 8, 16, 9), make(native, 2, 24, 32, 125), make(native, 3, 100, 256, 9)]
    per = [wrong_sets(o, [], 2, [1, o.rows - 1], j) for j, o in enumerate(clean)]
    good = [inject(pos, o, p) for o, p in zip(clean, per)]
    wants = [expected(o, [], p) for o, p in zip(clean, per)]
    alone = check_fleet(pos, native, good, [[], [], []], wants)
    files, knowns, ws = [], [], []
    for j, o in enumerate(clean):
        files += [good[j], o]
        knowns += [[], list(range(o.enc - o.pre + 1))]
        ws += [wants[j], None]
    res = check_fleet(pos, native, files, knowns, ws)
    assert [r["status"] for r in res[1::2]] == [UNRECOVERABLE] * 3
    for a, b in zip(alone, res[0::2]):
        assert np.array_equal(a["col_status"], b["col_status"]) and np.array_equal(a["row_status"], b["row_status"])


def test_a_word_that_is_not_below_p(pos, native, gpu):
    """a 0xFF column that is not listed is status 2 (the single-file entry answers such a job inside the
    call), against 3 for a listed one; with the known ones past enc - pre the job alone is unrecoverable"""
    o = make(native, 1, 8, 16, 9)
    a = inject(pos, o, {2: [5]})
    a.elems[7, :] = FF
    b = a.copy()
    b.elems[[0, 1, 2, 3, 4, 6, 8], :] = FF
    c = inject(pos, make(native, 3, 100, 256, 9), {0: [1, 2, 3]})
    c.elems[200, 4] = FF
    res = check_fleet(pos, native, [a, o, b, c, a], [[], [], [9], [17], [7]])
    assert res[0]["col_status"][7] == 2 and res[0]["col_status"][5] == 1
    assert (res[0]["row_status"] == pos.LOCATE_ROW_NOT_EVALUATED).all()
    assert not res[1]["col_status"].any() and not res[1]["row_status"].any()
    assert res[2]["status"] == UNRECOVERABLE
    assert res[3]["col_status"][200] == 2 and res[3]["col_status"][17] == 3 and list(res[3]["col_status"][1:4]) == [1, 1, 1]
    assert res[4]["col_status"][7] == 3 and list(res[4]["row_status"]) == [0, 0, 1, 0, 0, 0, 0, 0, 0]


def test_jobs_of_one_workgroup_differ(pos, native):
    spec = [(1, 3, 7), (8, 2, 2), (15, 1, 0), (8, 3, 4), (3, 1, 6), (12, 2, 1), (8, 1, 3), (1, 2, 5)]   # pre, rows, known
    files, knowns, wants = [], [], []
    for k, (pre, rows, nk) in enumerate(spec):
        o = make(native, 900 + k, pre, 16, rows)
        kn = [int(c) for c in np.random.default_rng(k).permutation(16)[:min(nk, 16 - pre)]]
        N = 16 - pre - len(kn)
        per_row = wrong_sets(o, kn, N // 2, range(rows), k)
        files.append(inject(pos, o, per_row))
        knowns.append(kn)
        wants.append(expected(o, kn, per_row))
    tiles, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [16] * len(files),
                                    [len(k) for k in knowns])
    assert groups == 1 and set(tiles["workgroup"]) == {0} and set(tiles["job"]) == set(range(len(spec)))
    res = check_fleet(pos, native, files, knowns, wants)
    for f, kn, r in zip(files, knowns, res):
        rs, cs = reference(pos, f, kn)
        assert np.array_equal(r["row_status"], rs) and np.array_equal(r["col_status"], cs)


def mixed_fleet(pos, native, n, seed=257):
    rng = np.random.default_rng(seed)
    dims = [(1, 2), (8, 16), (24, 32), (15, 16), (128, 256), (100, 256), (512, 1024), (1023, 1024), (3, 4)]
    files, knowns, wants = [], [], []
    for j in range(n):
        pre, enc = dims[j % len(dims)]
        o = make(native, 500 + j % 18, pre, enc, int(rng.choice([0, 1, 7, 8, 9, 17])))
        room = enc - pre
        kn = [int(c) for c in rng.permutation(enc)[:(0, 0, 1, room // 3, room, room + 1)[j % 6]]]
        N = room - len(kn)
        t = 0 if N <= 0 else ts_of(N)[j % 5]
        per_row = wrong_sets(o, kn, t, range(j % 2, o.rows, 2), j) if N > 0 else {}
        files.append(inject(pos, o, per_row))
        knowns.append(kn)
        wants.append(None if N < 0 else expected(o, kn, per_row))
    return files, knowns, wants


def test_mixed_fleet_in_one_group(pos, native):
    files, knowns, wants = mixed_fleet(pos, native, 257)
    _, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                [len(k) for k in knowns])
    assert groups == 1
    res = check_fleet(pos, native, files, knowns, wants)
    assert [r["status"] for r in res] == [UNRECOVERABLE if len(k) > f.enc - f.pre else 0 for f, k in zip(files, knowns)]


def routed_fleet(pos, native):
    origs = [make(native, 200 + j, 128, 256, 40 + j) for j in range(30)]       # about twelve to a group
    origs.insert(11, make(native, 240, 128, 256, 600))                         # above the group
    origs.insert(20, make(native, 241, 1024, 2048, 5))                         # enc = 2048
    origs.insert(5, make(native, 242, 8, 16, 0))                               # an empty file between two
    files, knowns, wants = [], [], []
    for j, o in enumerate(origs):
        kn = [] if j % 3 else [int(c) for c in np.random.default_rng(j).permutation(o.enc)[:1 + j % 5]]
        per_row = wrong_sets(o, kn, (0, 1, 5, 40)[j % 4], range(0, o.rows, 3), j)
        files.append(inject(pos, o, per_row))
        knowns.append(kn)
        wants.append(expected(o, kn, per_row))
    return files, knowns, wants


def test_groups_and_routing(pos, native, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    files, knowns, wants = routed_fleet(pos, native)
    tiles, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                    [len(k) for k in knowns])
    routed = np.unique(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE])
    assert groups >= 4 and list(routed) == [12, 21]
    res = check_fleet(pos, native, files, knowns, [None if j in (12, 21) else w for j, w in enumerate(wants)])
    for j in (12, 21):
        assert np.array_equal(res[j]["col_status"], wants[j][1])
        assert (res[j]["row_status"] == pos.LOCATE_ROW_NOT_EVALUATED).all()


def test_regions_are_the_plans_groups(gpu, pos, native, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    files, knowns, wants = routed_fleet(pos, native)
    keep = [j for j in range(len(files)) if j not in (12, 21)]
    files, knowns, wants = [files[j] for j in keep], [knowns[j] for j in keep], [wants[j] for j in keep]
    _, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                [len(k) for k in knowns])
    assert groups >= 3
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        res = call(pos, files, knowns)
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert stats.get(REGION, (0.0, 0))[1] == groups
    assert not any(name.startswith("rs_locate") or name.startswith("erasure") for name in stats), sorted(stats)
    for r, w in zip(res, wants):
        assert np.array_equal(r["row_status"], w[0]) and np.array_equal(r["col_status"], w[1])


def test_four_host_threads(pos, native):
    fleets = [mixed_fleet(pos, native, 40, seed=t) for t in range(4)]
    want = [check_fleet(pos, native, *fl) for fl in fleets]
    got, errs = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                got[t] = call(pos, fleets[t][0], fleets[t][1])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for t in range(4):
        for g, w in zip(got[t], want[t]):
            assert g["status"] == w["status"]
            if not g["status"]:
                assert np.array_equal(g["col_status"], w["col_status"]) and np.array_equal(g["row_status"], w["row_status"])


def test_a_recycled_pool_changes_nothing(pos, native):
    """the mixed queue in a fresh process whose device pool hands out blocks prefilled with 0xA5, and again
    with 0x00: every output byte has one writer and nothing relies on a cleared arena"""
    outs = []
    for poison in ("0xA5", "0x00"):
        env = dict(os.environ, LCPC_POOL_POISON=poison)
        p = subprocess.run([sys.executable, os.path.join(HERE, "_pos_group_locate_child.py")], env=env,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(p.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1] and outs[0].startswith("digest ")
    files, knowns, wants = mixed_fleet(pos, native, 120, seed=11)
    import hashlib
    h = hashlib.sha256()
    for r in call(pos, files, knowns) + call(pos, files[::-1], knowns[::-1]):
        h.update(repr(r["status"]).encode())
        if not r["status"]:
            h.update(r["col_status"].tobytes() + r["row_status"].tobytes())
    assert outs[0] == "digest " + h.hexdigest()
