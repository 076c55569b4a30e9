"""GPU: the grouped scrub of stored files (lcpc_pos_scrub_files_grouped).  Files are made
with lcpc_pos_encode_file into images prefilled with 0xA5 (capacity 2 rows + 3, so the rows past
rows_written hold garbage that must never be read), copies are damaged, and every answer is compared
with what the test did to the file, with lcpc_pos_scrub_porenc / lcpc_pos_locate_porenc per file and with
MerkleTree.new -- never with the grouped call itself.  Every comparison is exact."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REGION = "pos_group_scrub"
FILL = 0xA5
ROWS = (0, 1, 7, 8, 9, 124, 125, 252, 253, 1021)   # the tile seam, and the rows at which a leaf gains a chunk
DIMS = [(p, 1 << le) for le in range(1, 11) for p in sorted({1, max((1 << le) // 2, 1), (1 << le) - 1})] + \
    [(24, 32), (100, 256)]


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

    def __init__(self, img, tree, pre, enc, rows, cap, root=None):
        self.img, self.tree, self.pre, self.enc, self.rows, self.cap = img, tree, pre, enc, rows, cap
        self.root = tree[-1].tobytes() if root is None else root

    def copy(self):
        return Stored(self.img.copy(), self.tree.copy(), self.pre, self.enc, self.rows, self.cap, self.root)

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
        _made[key] = (Stored(img, tree, pre, enc, rows, cap), data)
    return _made[key][0]


def single_scrub(native, f, leaves):
    status, digests, n_bad = np.zeros(f.enc, np.uint8), np.zeros((f.enc, 32), np.uint8), C.c_size_t()
    lv = np.ascontiguousarray(leaves)
    assert native.load().lcpc_pos_scrub_porenc(u8(f.img), f.enc, f.rows, f.cap, u8(lv), u8(digests), u8(status),
                                               C.byref(n_bad)) == 0
    return status, digests, n_bad.value


def single_dirty_rows(native, f):
    status, nb, nd, nu = np.zeros(f.enc, np.uint8), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert native.load().lcpc_pos_locate_porenc(u8(f.img), f.pre, f.enc, f.rows, f.cap, None, 0, u8(status), C.byref(nb),
                                                C.byref(nd), C.byref(nu)) == 0
    return nd.value


def check_fleet(pos, native, merkle, files, tree_digests=None, with_roots=True):
    """the grouped call over `files` against the per-file entries and MerkleTree.new; returns its results.
    tree_digests: per file None (the whole tree), 0 or 'enc'."""
    n = len(files)
    kinds = [None] * n if tree_digests is None else tree_digests
    trees = []
    for f, k in zip(files, kinds):
        trees.append(f.tree if k is None else None if k == 0 else f.tree[:f.enc])
    roots = [f.root if with_roots else None for f in files]
    res = pos.scrub_files_grouped([f.img for f in files], [f.pre for f in files], [f.enc for f in files],
                                  [f.rows for f in files], [f.cap for f in files], trees, roots, want_digests=True)
    assert len(res) == n
    for j, (f, k, r) in enumerate(zip(files, kinds, res)):
        at = (j, f.pre, f.enc, f.rows, k)
        leaves = np.zeros((f.enc, 32), np.uint8) if k == 0 else f.tree[:f.enc]
        status, digests, n_bad = single_scrub(native, f, leaves)
        if k == 0:                                  # nothing to compare with: 0 or 2 only
            status = np.where(status == 1, 0, status).astype(np.uint8)
            n_bad = int((status != 0).sum())
            assert set(np.unique(r["status"])) <= {0, 2}, at
        assert np.array_equal(r["status"], status), at
        assert np.array_equal(r["digests"], digests), at
        assert r["n_bad"] == n_bad, at
        if (status == 2).any():
            assert r["n_dirty_rows"] is None, at
            assert not r["digests"][status == 2].any(), at
        else:
            assert r["n_dirty_rows"] == single_dirty_rows(native, f), at
        if k is None:
            assert r["tree_consistent"] == (merkle.new(f.tree[:f.enc]) == merkle(f.tree)), at
            assert r["root_ok"] == ((f.tree[-1].tobytes() == f.root) if with_roots else None), at
        else:
            assert r["tree_consistent"] is None and r["root_ok"] is None, at
    return res


def assert_clean(r, f, at=None):
    assert not r["status"].any() and r["n_bad"] == 0 and r["n_dirty_rows"] == 0, at
    assert np.array_equal(r["digests"], f.tree[:f.enc]), at
    assert r["tree_consistent"] is True and r["root_ok"] is True, at


def test_every_length_clean(pos, native, merkle, oracle):
    """every row length the kernel dispatches, at the three pres of each, the rows cycling through the seams"""
    files = [make(native, 100 + i, p, e, ROWS[i % len(ROWS)]) for i, (p, e) in enumerate(DIMS)]
    tiles, groups = pos.scrub_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files])
    assert groups == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any()
    res = check_fleet(pos, native, merkle, files)
    for j, (r, f) in enumerate(zip(res, files)):
        assert_clean(r, f, j)
    # the files are what the CPU oracle writes, so a damage below changes what the encode put there
    for i in (3, 28):
        f, data = _made[(100 + i, *DIMS[i], ROWS[i % len(ROWS)], 3)]
        o_img, o_tree, o_rows, _ = oracle.pos_encode_file(bytes(data), f.pre, f.enc, f.cap)
        assert o_rows == f.rows and o_tree == f.tree.tobytes()
        assert np.array_equal(np.frombuffer(o_img, "<u8").reshape(f.enc, f.cap)[:, :f.rows], f.elems[:, :f.rows])


@pytest.mark.parametrize("pre,enc", [(8, 16), (24, 32), (100, 256)])
def test_tile_and_chunk_seams(pos, native, merkle, pre, enc):
    files = [make(native, 7 * rows + pre, pre, enc, rows) for rows in ROWS]
    res = check_fleet(pos, native, merkle, files)
    for r, f in zip(res, files):
        assert_clean(r, f, f.rows)
    # one wrong element in the last row of each, and in the first: that row alone is dirty
    bad = [f.copy() for f in files if f.rows]
    for k, f in enumerate(bad):
        f.elems[k % enc, f.rows - 1] ^= np.uint64(1 << (k % 60))
        f.elems[(k + 5) % enc, 0] ^= np.uint64(2)
    res = check_fleet(pos, native, merkle, bad)
    for k, (r, f) in enumerate(zip(res, bad)):
        cols = sorted({k % enc, (k + 5) % enc})
        assert list(np.flatnonzero(r["status"])) == cols and set(r["status"][cols]) == {1}, f.rows
        assert r["n_dirty_rows"] == (1 if f.rows == 1 else 2), f.rows


def neighbours(native):
    return [make(native, 1, 8, 16, 9), make(native, 2, 24, 32, 125), make(native, 3, 100, 256, 9),
            make(native, 4, 1, 2, 7), make(native, 5, 512, 1024, 8)]


def run_damaged(pos, native, merkle, bad, **kw):
    """every damaged file between clean neighbours, all in one group; the neighbours stay clean"""
    clean = neighbours(native)
    files = []
    for k, f in enumerate(bad):
        files += [clean[k % len(clean)], f]
    files.append(clean[-1])
    res = check_fleet(pos, native, merkle, files, **kw)
    for j in range(0, len(files), 2):
        assert_clean(res[j], files[j], j)
    return [res[j] for j in range(1, len(files), 2)]


def test_one_flipped_bit(pos, native, merkle):
    P = pos.FT63_MODULUS
    bad, where = [], []
    for k, base in enumerate(neighbours(native) + [make(native, 6, 24, 32, 1021)]):
        f = base.copy()
        c, r = (3 * k + 1) % f.enc, (5 * k + 2) % f.rows
        f.elems[c, r] ^= np.uint64(1 << (7 * k % 61))
        assert int(f.elems[c, r]) < P and f.elems[c, r] != base.elems[c, r]
        bad.append(f)
        where.append(c)
    for r, f, c in zip(run_damaged(pos, native, merkle, bad), bad, where):
        assert list(np.flatnonzero(r["status"])) == [c] and r["status"][c] == 1 and r["n_bad"] == 1
        assert r["n_dirty_rows"] == 1 and r["tree_consistent"] is True and r["root_ok"] is True


def test_noncanonical_column(pos, native, merkle):
    bad = []
    for k, base in enumerate(neighbours(native)):
        f = base.copy()
        f.elems[(k + 1) % f.enc, :f.rows] = np.uint64(0xFFFFFFFFFFFFFFFF)
        bad.append(f)
    for k, (r, f) in enumerate(zip(run_damaged(pos, native, merkle, bad), bad)):
        c = (k + 1) % f.enc
        assert list(np.flatnonzero(r["status"])) == [c] and r["status"][c] == 2 and r["n_bad"] == 1
        assert not r["digests"][c].any() and r["n_dirty_rows"] is None
        assert r["tree_consistent"] is True and r["root_ok"] is True


def test_damaged_tree_only(pos, native, merkle):
    base = neighbours(native)
    leaf, parent, root = base[1].copy(), base[2].copy(), base[0].copy()
    leaf.tree[5, 3] ^= 0x10                      # a stored leaf
    parent.tree[parent.enc + 7, 31] ^= 1         # a stored parent that is not the root
    root.tree[-1, 0] ^= 0x80                     # the stored root (expected_root stays the original)
    r_leaf, r_parent, r_root = run_damaged(pos, native, merkle, [leaf, parent, root])
    assert list(np.flatnonzero(r_leaf["status"])) == [5] and r_leaf["status"][5] == 1 and r_leaf["n_dirty_rows"] == 0
    assert r_leaf["tree_consistent"] is False and r_leaf["root_ok"] is True
    assert not r_parent["status"].any() and r_parent["n_dirty_rows"] == 0
    assert r_parent["tree_consistent"] is False and r_parent["root_ok"] is True
    assert not r_root["status"].any() and r_root["n_dirty_rows"] == 0
    assert r_root["tree_consistent"] is False and r_root["root_ok"] is False


def test_rows_past_the_data_are_not_read(pos, native, merkle):
    bad = []
    for base in neighbours(native):
        f = base.copy()
        f.elems[:, f.rows:] ^= np.uint64(0x5A5A5A5A5A5A5A5A)
        f.elems[1, f.rows] = np.uint64(0xFFFFFFFFFFFFFFFF)
        bad.append(f)
    for r, f in zip(run_damaged(pos, native, merkle, bad), bad):
        assert_clean(r, f)


def test_consistent_forgery_is_seen_by_the_code_alone(pos, native, merkle):
    """a column of random canonical values with its leaf, parents and root recomputed: every hash agrees,
    only the row code knows"""
    P = pos.FT63_MODULUS
    bad = []
    for k, base in enumerate(neighbours(native)):
        f = base.copy()
        c = (2 * k + 1) % f.enc
        f.elems[c, :f.rows] = np.random.default_rng(50 + k).integers(0, P, f.rows, dtype=np.uint64)
        assert (f.elems[c, :f.rows] != base.elems[c, :base.rows]).all()
        _, digests, _ = single_scrub(native, f, f.tree[:f.enc])
        f.tree = merkle.new(digests).digests.copy()
        assert f.tree[-1].tobytes() != base.root and f.root == base.root
        bad.append(f)
    for r, f in zip(run_damaged(pos, native, merkle, bad), bad):
        assert not r["status"].any() and r["n_bad"] == 0 and r["tree_consistent"] is True
        assert r["n_dirty_rows"] == f.rows and r["root_ok"] is False
    for f in bad:                                # the owner who trusts the new root sees nothing but the code
        f.root = f.tree[-1].tobytes()
    for r, f in zip(run_damaged(pos, native, merkle, bad), bad):
        assert not r["status"].any() and r["tree_consistent"] is True and r["root_ok"] is True
        assert r["n_dirty_rows"] == f.rows


def test_more_damage_than_the_code_corrects_is_a_report(pos, native, merkle):
    bad, cols = [], []
    for base in neighbours(native)[:3]:
        f = base.copy()
        n = f.enc - f.pre + 1
        f.elems[:n, 0] ^= np.uint64(4)
        assert (f.elems[:n, 0] < pos.FT63_MODULUS).all()
        bad.append(f)
        cols.append(n)
    for r, f, n in zip(run_damaged(pos, native, merkle, bad), bad, cols):
        assert list(np.flatnonzero(r["status"])) == list(range(n)) and r["n_bad"] == n
        assert r["n_dirty_rows"] == 1


def test_without_a_tree_and_with_leaves_only(pos, native, merkle):
    base = neighbours(native)
    flipped, ff = base[0].copy(), base[1].copy()
    flipped.elems[2, 1] ^= np.uint64(1)
    ff.elems[4, :ff.rows] = np.uint64(0xFFFFFFFFFFFFFFFF)
    files = [base[0], flipped, base[2], ff, base[4], base[3]]
    none = check_fleet(pos, native, merkle, files, tree_digests=[0] * 6)
    assert [r["n_bad"] for r in none] == [0, 0, 0, 1, 0, 0] and none[3]["status"][4] == 2
    assert [r["n_dirty_rows"] for r in none] == [0, 1, 0, None, 0, 0]
    lv = check_fleet(pos, native, merkle, files, tree_digests=["enc"] * 6)
    assert [r["n_bad"] for r in lv] == [0, 1, 0, 1, 0, 0] and lv[1]["status"][2] == 1
    mixed = check_fleet(pos, native, merkle, files, tree_digests=[None, 0, "enc", None, 0, "enc"], with_roots=False)
    assert [r["tree_consistent"] for r in mixed] == [True, None, None, True, None, None]
    assert all(r["root_ok"] is None for r in mixed)
    # digests are optional
    r = pos.scrub_files_grouped([f.img for f in files], [f.pre for f in files], [f.enc for f in files],
                                [f.rows for f in files], [f.cap for f in files], [f.tree for f in files])
    assert all(o["digests"] is None for o in r) and [o["n_bad"] for o in r] == [0, 1, 0, 1, 0, 0]


def test_mixed_fleet_in_one_group(pos, native, merkle):
    """257 jobs of nine dims in one group, every seventh damaged in a way of its own"""
    rng = np.random.default_rng(257)
    dims = [(1, 2), (8, 16), (24, 32), (15, 16), (128, 256), (100, 256), (512, 1024), (1023, 1024), (3, 4)]
    files, want = [], []
    for j in range(257):
        pre, enc = dims[j % len(dims)]
        f = make(native, 500 + j % 18, pre, enc, int(rng.choice([0, 1, 7, 8, 9, 17])))
        kind = (j // 7) % 3 if j % 7 == 3 and f.rows else None
        if kind is not None:
            f = f.copy()
            c, r = j % enc, j % f.rows
            if kind == 0:
                f.elems[c, r] ^= np.uint64(1 << (j % 20))
            elif kind == 1:
                f.elems[c, :f.rows] = np.uint64(0xFFFFFFFFFFFFFFFF)
            else:
                f.tree[enc + j % (enc - 1), j % 32] ^= 1
        files.append(f)
        want.append(kind)
    _, groups = pos.scrub_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files])
    assert groups == 1
    res = check_fleet(pos, native, merkle, files)
    for j, (r, f, kind) in enumerate(zip(res, files, want)):
        if kind is None:
            assert_clean(r, f, j)
        elif kind == 0:
            assert list(np.flatnonzero(r["status"])) == [j % f.enc] and r["n_dirty_rows"] == 1, j
        elif kind == 1:
            assert r["status"][j % f.enc] == 2 and r["n_bad"] == 1 and r["n_dirty_rows"] is None, j
        else:
            assert r["n_bad"] == 0 and r["n_dirty_rows"] == 0 and r["tree_consistent"] is False, j


def test_groups_and_routing(pos, native, merkle, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    files = [make(native, 200 + j, 128, 256, 40 + j) for j in range(30)]       # about twelve to a group
    files.insert(11, make(native, 240, 128, 256, 600))                         # above the group
    files.insert(20, make(native, 241, 1024, 2048, 5))                         # enc = 2048
    files.insert(5, make(native, 242, 8, 16, 0))                               # an empty file between two
    tiles, groups = pos.scrub_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files])
    routed = np.unique(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE])
    assert groups >= 4 and list(routed) == [12, 21]
    res = check_fleet(pos, native, merkle, files)
    for j, (r, f) in enumerate(zip(res, files)):
        assert_clean(r, f, j)
    # the same with findings in the routed jobs and in a grouped one
    files = [f.copy() for f in files]
    files[12].elems[9, 599] ^= np.uint64(1)
    files[21].elems[2047, 0] ^= np.uint64(1)
    files[21].tree[2048 + 3, 0] ^= 1
    files[13].elems[0, 0] ^= np.uint64(1)
    res = check_fleet(pos, native, merkle, files)
    assert [j for j, r in enumerate(res) if r["n_bad"]] == [12, 13, 21]
    assert [res[j]["n_dirty_rows"] for j in (12, 13, 21)] == [1, 1, 1]
    assert res[21]["tree_consistent"] is False and res[21]["root_ok"] is True and res[12]["tree_consistent"] is True
    # routed jobs without a tree, and with leaves only
    check_fleet(pos, native, merkle, files[10:23], tree_digests=[0, "enc"] * 6 + [0])


def test_many_jobs_few_launches(gpu, pos, native, merkle):
    distinct = [make(native, 300 + j, 8, 16, 1, cut=j % 3) for j in range(50)]
    files = [distinct[j % 50] for j in range(1000)]
    files[777] = files[777].copy()
    files[777].elems[3, 0] ^= np.uint64(1)
    _, groups = pos.scrub_plan([1] * 1000, [8] * 1000, [16] * 1000)
    assert groups == 1
    args = ([f.img for f in files], [8] * 1000, [16] * 1000, [1] * 1000, [f.cap for f in files],
            [f.tree for f in files], [f.root for f in files])
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        res = pos.scrub_files_grouped(*args, want_digests=True)
        ms, count = gpu.prof_stats().get(REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert 1 <= count <= groups
    assert [j for j, r in enumerate(res) if r["n_bad"] or r["n_dirty_rows"]] == [777]
    assert list(np.flatnonzero(res[777]["status"])) == [3] and res[777]["n_dirty_rows"] == 1
    for j in list(range(0, 1000, 50)) + [777]:
        f = files[j]
        status, digests, n_bad = single_scrub(native, f, f.tree[:16])
        assert np.array_equal(res[j]["status"], status) and np.array_equal(res[j]["digests"], digests)
        assert res[j]["n_bad"] == n_bad and res[j]["n_dirty_rows"] == single_dirty_rows(native, f)
        assert res[j]["tree_consistent"] is True and res[j]["root_ok"] is True


def test_four_host_threads(pos, native, merkle):
    fleets = []
    for t in range(4):
        fl = [make(native, 400 + 10 * t + j, 24, 32, 5 + j) for j in range(10)]
        fl[t] = fl[t].copy()
        fl[t].elems[t, t] ^= np.uint64(1)
        fl[t + 4] = fl[t + 4].copy()
        fl[t + 4].tree[40 + t, 1] ^= 1
        fleets.append(fl)

    def call(fl):
        return pos.scrub_files_grouped([f.img for f in fl], [24] * 10, [32] * 10, [f.rows for f in fl],
                                       [f.cap for f in fl], [f.tree for f in fl], [f.root for f in fl], want_digests=True)

    want = [check_fleet(pos, native, merkle, fl) for fl in fleets]
    got, errs = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                got[t] = call(fleets[t])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for t in range(4):
        assert [r["n_bad"] for r in got[t]] == [1 if j == t else 0 for j in range(10)]
        assert [r["tree_consistent"] for r in got[t]] == [j != t + 4 for j in range(10)]
        for g, w in zip(got[t], want[t]):
            assert np.array_equal(g["status"], w["status"]) and np.array_equal(g["digests"], w["digests"])
            assert {k: g[k] for k in g if k not in ("status", "digests")} == \
                {k: w[k] for k in w if k not in ("status", "digests")}
