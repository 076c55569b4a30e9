"""GPU: the grouped repair of stored files (lcpc_pos_repair_files_grouped).  Files are made
with lcpc_pos_encode_file into images prefilled with 0xA5 (capacity 2 rows + 3), copies get their listed
columns overwritten with 0xFF words, and every answer is compared with the PRE-DAMAGE image and tree, with
lcpc_pos_repair_columns on the same damaged image and with MerkleTree.new -- never with the grouped call
itself.  Every comparison is exact."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REGION = "pos_group_repair"
FILL = 0xA5
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
UNRECOVERABLE = 36
ROWS = (0, 1, 7, 8, 9, 124, 125, 253, 1021)   # the tile seam, and the rows at which a leaf gains a chunk
DIMS = [(p, 1 << le) for le in range(1, 11) for p in sorted({1, max((1 << le) // 2, 1), (1 << le) - 1})] + \
    [(24, 32), (100, 256)]
KINDS = ("none", "first", "last", "run", "scattered", "full")


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


@pytest.fixture(scope="module")
def merkle(gpu):
    from lcpc_proof_of_storage_amd.pos_files import MerkleTree
    return MerkleTree


def u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None


class Stored:
    """a stored file as the grouped call takes it; copy() for a copy to damage"""

    def __init__(self, img, tree, pre, enc, rows, cap):
        self.img, self.tree, self.pre, self.enc, self.rows, self.cap = img, tree, pre, enc, rows, cap

    def copy(self):
        return Stored(self.img.copy(), self.tree.copy(), self.pre, self.enc, self.rows, self.cap)

    @property
    def elems(self):
        return self.img.view("<u8").reshape(self.enc, self.cap)


_made = {}


def make(native, seed, pre, enc, rows, cut=3):
    """lcpc_pos_encode_file of a random file of `rows` rows (the last one `cut` bytes short); shared, never
    changed: tests damage copies"""
    key = (seed, pre, enc, rows, cut)
    if key not in _made:
        lib = native.load()
        data = np.random.default_rng(seed).integers(0, 256, max(rows * 7 * pre - cut, 0), dtype=np.uint8)
        cap = 2 * rows + 3
        img = np.full(enc * cap * 8, FILL, np.uint8)
        tree = np.zeros((2 * enc - 1, 32), np.uint8)
        got = C.c_size_t()
        assert lib.lcpc_pos_encode_file(u8(data), data.size, pre, enc, cap, u8(img), u8(tree), C.byref(got)) == 0
        assert got.value == rows
        _made[key] = Stored(img, tree, pre, enc, rows, cap)
    return _made[key]


def erasures(kind, pre, enc, seed=0):
    """the erasure sets of the issue, every one within the code's redundancy"""
    room = enc - pre
    if kind == "none":
        return []
    if kind == "first":
        return [0]
    if kind == "last":
        return [enc - 1]
    if kind == "run":
        n = max(1, min(room, 16, enc // 2))
        lo = (seed * 7) % (enc - n + 1)
        return list(range(lo, lo + n))
    if kind == "scattered":
        n = max(1, min(room, 5))
        return [int(c) for c in np.random.default_rng(seed).permutation(enc)[:n]]
    return [int(c) for c in np.random.default_rng(seed + 1).permutation(enc)[:room]]   # exactly enc - pre: no degree check


def damaged(f, bad):
    """a copy with the listed columns, slack included, overwritten by words that are not < p"""
    g = f.copy()
    if len(bad):
        g.elems[list(bad), :] = FF
    return g


def single_repair(native, f, bad):
    b = np.asarray(bad, np.uint64)
    cols, dig = np.zeros((b.size, f.rows), np.uint64), np.zeros((b.size, 32), np.uint8)
    st = native.load().lcpc_pos_repair_columns(u8(f.img), f.pre, f.enc, f.rows, f.cap,
                                               b.ctypes.data_as(C.POINTER(C.c_uint64)) if b.size else None, b.size,
                                               u8(cols.view(np.uint8).reshape(-1)), u8(dig.reshape(-1)), None)
    assert st in (0, UNRECOVERABLE)
    return st, cols, dig


def call(pos, files, bads, leaves=None, **kw):
    return pos.repair_files_grouped([f.img for f in files], [f.pre for f in files], [f.enc for f in files],
                                    [f.rows for f in files], [f.cap for f in files], bads, leaves, **kw)


def check_fleet(pos, native, merkle, files, bads, origs=None, leaves="tree", single=True):
    """the grouped call over `files` against the pre-damage files `origs` (where the job is expected to
    succeed), lcpc_pos_repair_columns and MerkleTree.new; returns its results.  leaves: 'tree' (the
    pre-damage leaves), 'zeros' or None."""
    n = len(files)
    origs = [None] * n if origs is None else origs
    lv = [None if leaves is None else (o or f).tree[:f.enc] if leaves == "tree" else np.zeros((f.enc, 32), np.uint8)
          for f, o in zip(files, origs)]
    res = call(pos, files, bads, None if leaves is None else lv, want_tree=leaves is not None)
    assert len(res) == n
    for j, (f, bad, o, r) in enumerate(zip(files, bads, origs, res)):
        at = (j, f.pre, f.enc, f.rows, len(bad))
        if single:
            st, cols, dig = single_repair(native, f, bad)
            assert r["status"] == st, at
        if o is not None:
            assert r["status"] == 0, at
        if r["status"]:
            assert r["cols"] is None and r["digests"] is None and r["tree"] is None and r["root"] is None, at
            continue
        assert r["cols"].shape == (len(bad), f.rows) and r["digests"].shape == (len(bad), 32), at
        if single:
            assert np.array_equal(r["cols"], cols), at
            assert np.array_equal(r["digests"], dig), at
        if o is not None and len(bad):
            assert np.array_equal(r["cols"], o.elems[list(bad), :f.rows]), at
            assert np.array_equal(r["digests"], o.tree[list(bad)]), at
        if leaves is None:
            assert r["tree"] is None and r["root"] is None, at
        else:
            want = lv[j].copy()
            if len(bad):
                want[list(bad)] = o.tree[list(bad)] if o is not None else dig
            t = merkle.new(want)
            assert np.array_equal(r["tree"], t.digests), at
            assert r["root"] == t.root(), at
    return res


def test_every_length_and_erasure_set(pos, native, merkle):
    """every row length the kernel dispatches, at the three pres of each, the rows cycling through the
    seams and the erasure sets through their kinds"""
    origs, bads = [], []
    for i, (p, e) in enumerate(DIMS):
        origs.append(make(native, 100 + i, p, e, ROWS[(i + 1) % len(ROWS)]))
        bads.append(erasures(KINDS[i % len(KINDS)], p, e, i))
    for i, (p, e) in enumerate(DIMS[::3]):               # every length once more at the full erasure count
        origs.append(make(native, 100 + 3 * i, p, e, ROWS[(3 * i + 1) % len(ROWS)]))
        bads.append(erasures("full", p, e, i))
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    tiles, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                    [len(b) for b in bads])
    assert groups == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any()
    check_fleet(pos, native, merkle, files, bads, origs)


def test_the_largest_tile_and_the_longest_locator(pos, native, merkle):
    f = make(native, 7, 512, 1024, 8)
    bad = erasures("full", 512, 1024, 3)
    assert len(bad) == 512
    check_fleet(pos, native, merkle, [damaged(f, bad)], [bad], [f])


@pytest.mark.parametrize("pre,enc", [(8, 16), (24, 32), (100, 256)])
def test_tile_and_chunk_seams(pos, native, merkle, pre, enc):
    origs = [make(native, 7 * rows + pre, pre, enc, rows) for rows in ROWS for _ in KINDS]
    bads = [erasures(k, pre, enc, rows) for rows in ROWS for k in KINDS]
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    check_fleet(pos, native, merkle, files, bads, origs)


def test_jobs_of_one_workgroup_differ_in_pre_and_erasures(pos, native, merkle):
    """what the per-file decoder cannot get wrong and this kernel can: the tiles of one workgroup belong to
    jobs with different pre, different erasure sets and different row counts"""
    spec = [(1, 3, "full"), (8, 2, "run"), (15, 1, "last"), (8, 3, "none"), (3, 1, "scattered"), (12, 2, "full"),
            (8, 1, "first"), (1, 2, "scattered")]
    origs = [make(native, 900 + k, pre, 16, rows) for k, (pre, rows, _) in enumerate(spec)]
    bads = [erasures(kind, pre, 16, k) for k, (pre, _, kind) in enumerate(spec)]
    assert len({tuple(sorted(b)) for b in bads}) == len(bads)
    tiles, groups = pos.repair_plan([f.rows for f in origs], [f.pre for f in origs], [16] * len(origs),
                                    [len(b) for b in bads])
    assert groups == 1 and set(tiles["workgroup"]) == {0} and set(tiles["job"]) == set(range(len(spec)))
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    check_fleet(pos, native, merkle, files, bads, origs)
    # the same at 256 points, where every tile has a workgroup, and at 4 points with 11-row jobs
    for enc, pres, rows in ((256, (1, 100, 128, 255), 9), (4, (1, 2, 3), 11)):
        origs = [make(native, 920 + k, pre, enc, rows) for k, pre in enumerate(pres)]
        bads = [erasures(KINDS[1 + k % 5], pre, enc, k) for k, pre in enumerate(pres)]
        check_fleet(pos, native, merkle, [damaged(f, b) for f, b in zip(origs, bads)], bads, origs)


def test_listed_columns_are_never_read(pos, native, merkle):
    origs = [make(native, 1, 8, 16, 9), make(native, 2, 24, 32, 125), make(native, 3, 100, 256, 9)]
    bads = [[3, 0, 15], [31], list(range(40, 56))]
    a = [damaged(f, b) for f, b in zip(origs, bads)]
    b = [f.copy() for f in origs]
    for g, bad in zip(b, bads):
        g.elems[bad, :] ^= np.uint64(0x0123456789ABCDEF)
    ra = check_fleet(pos, native, merkle, a, bads, origs)
    rb = check_fleet(pos, native, merkle, b, bads, origs, single=False)
    for x, y in zip(ra, rb):
        assert np.array_equal(x["cols"], y["cols"]) and np.array_equal(x["digests"], y["digests"])
        assert np.array_equal(x["tree"], y["tree"]) and x["root"] == y["root"]


def test_a_sound_listed_column_repairs_to_itself(pos, native, merkle):
    origs = [make(native, 1, 8, 16, 9), make(native, 5, 512, 1024, 8), make(native, 4, 1, 2, 7)]
    bads = [[5, 6], [1000], [1]]
    res = check_fleet(pos, native, merkle, origs, bads, origs)
    for r, f in zip(res, origs):
        assert np.array_equal(r["tree"], f.tree) and r["root"] == f.tree[-1].tobytes()


def neighbours(native):
    return [make(native, 1, 8, 16, 9), make(native, 2, 24, 32, 125), make(native, 3, 100, 256, 9),
            make(native, 4, 1, 2, 7), make(native, 5, 512, 1024, 8)]


def test_a_failed_job_leaves_its_neighbours_alone(pos, native, merkle):
    P = pos.FT63_MODULUS
    clean = neighbours(native)
    cbad = [[2], [0, 31], list(range(100, 110)), [0], [77, 1023]]
    alone = check_fleet(pos, native, merkle, [damaged(f, b) for f, b in zip(clean, cbad)], cbad, clean)
    failing = []
    # more listed columns than the code can restore
    f = clean[0]
    failing.append((f, list(range(f.enc - f.pre + 1))))
    # a flipped bit in a column that is not listed, with room for the degree check
    for k, base in enumerate((clean[1], clean[2], clean[4])):
        f = base.copy()
        c, r = 7 + k, (5 * k + 2) % f.rows
        f.elems[c, r] ^= np.uint64(1 << (7 * k % 61))
        assert int(f.elems[c, r]) < P
        failing.append((f, [c + 1, 0]))
    # a word that is not < p in a column that is not listed
    for k, base in enumerate((clean[0], clean[3], clean[2])):
        f = base.copy()
        f.elems[(k + 1) % f.enc, f.rows - 1] = FF
        failing.append((f, [] if k == 1 else [(k + 2) % f.enc]))
    files, bads, origs = [], [], []
    for k, (f, b) in enumerate(failing):
        files += [damaged(clean[k % 5], cbad[k % 5]), f]
        bads += [cbad[k % 5], b]
        origs += [clean[k % 5], None]
    files.append(damaged(clean[4], cbad[4]))
    bads.append(cbad[4])
    origs.append(clean[4])
    res = check_fleet(pos, native, merkle, files, bads, origs)
    assert [r["status"] for r in res[1::2]] == [UNRECOVERABLE] * len(failing)
    for j in range(0, len(files), 2):       # every neighbour's outputs are what they are without the failures
        w = alone[(j // 2) % 5] if j + 1 < len(files) else alone[4]
        for key in ("cols", "digests", "tree"):
            assert np.array_equal(res[j][key], w[key]), (j, key)
        assert res[j]["root"] == w["root"]


def test_trees_with_and_without_leaves(pos, native, merkle):
    origs = neighbours(native) + [make(native, 6, 8, 16, 0)]
    bads = [[2], [0, 31], list(range(100, 110)), [0], [77, 1023], [4, 9]]
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    check_fleet(pos, native, merkle, files, bads, origs, leaves="tree")
    check_fleet(pos, native, merkle, files, bads, origs, leaves="zeros")
    check_fleet(pos, native, merkle, files, bads, origs, leaves=None)
    # leaves for some jobs only, and no columns wanted
    lv = [f.tree[:f.enc] if j % 2 else None for j, f in enumerate(origs)]
    res = call(pos, files, bads, lv, want_cols=False, want_tree=True)
    for j, (r, f, b) in enumerate(zip(res, origs, bads)):
        assert r["status"] == 0 and r["cols"] is None and np.array_equal(r["digests"], f.tree[b])
        if j % 2:
            assert np.array_equal(r["tree"], f.tree) and r["root"] == f.tree[-1].tobytes()
        else:
            assert r["tree"] is None and r["root"] is None


def test_mixed_fleet_in_one_group(pos, native, merkle):
    """257 jobs of nine dims in one group, every seventh unrecoverable in a way of its own"""
    rng = np.random.default_rng(257)
    dims = [(1, 2), (8, 16), (24, 32), (15, 16), (128, 256), (100, 256), (512, 1024), (1023, 1024), (3, 4)]
    files, bads, origs, want = [], [], [], []
    for j in range(257):
        pre, enc = dims[j % len(dims)]
        o = make(native, 500 + j % 18, pre, enc, int(rng.choice([0, 1, 7, 8, 9, 17])))
        bad = erasures(KINDS[j % len(KINDS)], pre, enc, j)
        f = damaged(o, bad)
        fails = j % 7 == 3 and o.rows > 0
        if fails:
            free = [c for c in range(enc) if c not in bad]
            if (j // 7) % 2 == 0 or len(bad) == enc - pre:
                f.elems[free[j % len(free)], j % o.rows] = FF          # not < p
            else:
                f.elems[free[j % len(free)], j % o.rows] ^= np.uint64(1 << (j % 20))
        files.append(f)
        bads.append(bad)
        origs.append(None if fails else o)
        want.append(UNRECOVERABLE if fails else 0)
    _, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                [len(b) for b in bads])
    assert groups == 1
    res = check_fleet(pos, native, merkle, files, bads, origs)
    assert [r["status"] for r in res] == want


def test_groups_and_routing(pos, native, merkle, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    origs = [make(native, 200 + j, 128, 256, 40 + j) for j in range(30)]       # about twelve to a group
    origs.insert(11, make(native, 240, 128, 256, 600))                         # above the group
    origs.insert(20, make(native, 241, 1024, 2048, 5))                         # enc = 2048
    origs.insert(5, make(native, 242, 8, 16, 0))                               # an empty file between two
    bads = [erasures(KINDS[1 + j % 5], f.pre, f.enc, j) for j, f in enumerate(origs)]
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    tiles, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                    [len(b) for b in bads])
    routed = np.unique(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE])
    assert groups >= 4 and list(routed) == [12, 21]
    check_fleet(pos, native, merkle, files, bads, origs)
    check_fleet(pos, native, merkle, files[10:23], bads[10:23], origs[10:23], leaves=None)
    # a routed job that fails, and one that lists too much, leave the others alone
    files[21] = files[21].copy()
    files[21].elems[next(c for c in range(2048) if c not in bads[21]), 0] = FF
    origs[21] = None
    bads[12] = list(range(129))
    origs[12] = None
    res = check_fleet(pos, native, merkle, files, bads, origs)
    assert [j for j, r in enumerate(res) if r["status"]] == [12, 21]


def test_regions_are_the_plans_launches(gpu, pos, native, merkle, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    distinct = [make(native, 300 + j, 8, 16, 1, cut=j % 3) for j in range(50)]
    origs = [distinct[j % 50] for j in range(1000)] + [make(native, 200 + j, 128, 256, 40 + j) for j in range(30)]
    bads = [erasures(KINDS[j % len(KINDS)], f.pre, f.enc, j) for j, f in enumerate(origs)]
    bads[500] = list(range(9))                                                  # no device work
    files = [damaged(f, b) for f, b in zip(origs, bads)]
    _, groups = pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                [len(b) for b in bads])
    assert groups >= 3
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        res = call(pos, files, bads, [f.tree[:f.enc] for f in origs], want_tree=True)
        ms, count = gpu.prof_stats().get(REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert count == groups
    assert [j for j, r in enumerate(res) if r["status"]] == [500]
    for j, (r, o, b) in enumerate(zip(res, origs, bads)):
        if j == 500:
            continue
        assert np.array_equal(r["cols"], o.elems[b, :o.rows]) and np.array_equal(r["digests"], o.tree[b]), j
        assert np.array_equal(r["tree"], o.tree) and r["root"] == o.tree[-1].tobytes(), j


def test_four_host_threads(pos, native, merkle):
    fleets = []
    for t in range(4):
        origs = [make(native, 400 + 10 * t + j, 24, 32, 5 + j) for j in range(10)]
        bads = [erasures(KINDS[(t + j) % len(KINDS)], 24, 32, 10 * t + j) for j in range(10)]
        files = [damaged(f, b) for f, b in zip(origs, bads)]
        free = next(c for c in range(32) if c not in bads[t])
        files[t].elems[free, t] = FF
        fleets.append((files, bads, [None if j == t else o for j, o in enumerate(origs)],
                       [o.tree[:32] for o in origs]))
    want = [check_fleet(pos, native, merkle, fl[0], fl[1], fl[2]) for fl in fleets]
    got, errs = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                got[t] = call(pos, fleets[t][0], fleets[t][1], fleets[t][3], want_tree=True)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for t in range(4):
        assert [r["status"] for r in got[t]] == [UNRECOVERABLE if j == t else 0 for j in range(10)]
        for g, w in zip(got[t], want[t]):
            for key in ("cols", "digests", "tree"):
                assert np.array_equal(g[key], w[key])
            assert g["root"] == w["root"]
