"""GPU: the grouped ingest, scrub, repair and audit check of stored files whose column leaves have 255 to
313 BLAKE3 chunks, the depths at which their tree folds change instantiation.  The reference of every
comparison is the C oracle's encode of the same file (oracle.pos_encode_file), pure-Python BLAKE3
(read_ref) or, for the audit check, the single check pos.client_verify_evaluation -- never the grouped
call.  Every comparison is exact.

A launcher picks its fold from the largest chunk count of the staging group, so every fleet runs twice:
"shallow" holds the files of at most 256 chunks and "deep" all of them.  Dispatch sites reached, and the
chunk counts (rows) at which they are reached:

* pos_ingest.hip k_group_ingest_trees<8>: shallow, leaves of 1 (9 rows), 255 (32636), 256 with one
  element in the last chunk (32637) and 256 full chunks (32764: every level of the stack occupied);
  k_group_ingest_trees<16>: deep, the same plus 257 (32765, at two dims) and 313 (40000) chunks.
* pos_scrub.hip and pos_repair_group.hip, the leaf_fold_stack<8 / 16> callers: the same two fleets.
* pos_verify_group.hip k_group_leaf_finish<F, 8>: shallow, 1, 3, 255, 256 and 256 chunks;
  k_group_leaf_finish<F, 16>: deep, the same plus 257 and 313.
"""
import numpy as np
import pytest

import read_ref
from test_gpu_pos_group_verify import REGION as VERIFY_REGION
from test_gpu_pos_group_verify import Server, elems, names, same, single, with_column

pytestmark = pytest.mark.gpu
FT63 = 0
FILL = 0xA5
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
# Ft63 leaves (32 + 8 rows bytes) of 255 full chunks, 256 chunks with one element in the last, 256 full
# chunks, 257 chunks with a one-block last chunk, and 313 chunks
DEEP_ROWS = (32636, 32637, 32764, 32765, 40000)
# (rows, pre, enc): one file per DEEP_ROWS entry at (1, 2), the first 257-chunk shape at (8, 16), two 9-row files
DEEP = [(r, 1, 2) for r in DEEP_ROWS] + [(32765, 8, 16), (9, 8, 16), (9, 24, 32)]
SHALLOW = [s for s in DEEP if read_ref.n_chunks(s[0]) <= 256]
FLEETS = {"shallow": SHALLOW, "deep": DEEP}


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


class Stored:
    """a file as the oracle stores it: the image with `cap` rows per column (the rows past the data hold
    0xA5 bytes), the tree, and the data it was made from"""

    def __init__(self, data, img, tree, pre, enc, rows, cap):
        self.data, self.img, self.tree, self.pre, self.enc, self.rows, self.cap = data, img, tree, pre, enc, rows, cap

    def copy(self):
        return Stored(self.data, self.img.copy(), self.tree.copy(), self.pre, self.enc, self.rows, self.cap)

    @property
    def elems(self):
        return self.img.view("<u8").reshape(self.enc, self.cap)

    @property
    def root(self):
        return self.tree[-1].tobytes()


_made = {}


def make(oracle, rows, pre, enc):
    """oracle.pos_encode_file of a random file of `rows` rows, the last one 3 bytes short; made once and never
    changed: tests damage copies"""
    key = (rows, pre, enc)
    if key not in _made:
        data = np.random.default_rng(rows + enc).integers(0, 256, rows * 7 * pre - 3, dtype=np.uint8)
        cap = rows + 3
        o_img, o_tree, o_rows, o_cap = oracle.pos_encode_file(data.tobytes(), pre, enc, cap)
        assert (o_rows, o_cap) == (rows, cap)
        img = np.frombuffer(o_img, np.uint8).copy()
        img.view("<u8").reshape(enc, cap)[:, rows:] = np.uint64(int.from_bytes(bytes([FILL]) * 8, "little"))
        tree = np.frombuffer(o_tree, np.uint8).reshape(2 * enc - 1, 32).copy()
        _made[key] = Stored(data, img, tree, pre, enc, rows, cap)
    return _made[key]


def fleet(oracle, name):
    return [make(oracle, *s) for s in FLEETS[name]]


def deep_jobs(files):
    return [j for j, f in enumerate(files) if f.rows > 9]


def assert_one_group(pos, plan, files):
    """no job takes the single-file path and the deep jobs share their launch with the small ones"""
    tiles, groups = plan
    assert groups == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any()
    assert set(tiles["launch"].tolist()) == {0} and set(tiles["job"].tolist()) == set(range(len(files)))


# ---------------------------------------------------------------- ingest
@pytest.mark.parametrize("name", list(FLEETS))
def test_ingest(pos, oracle, name):
    """pos.encode_files_grouped_into of the fleet in one call: image (the rows past rows_written untouched),
    tree, root and rows_written against the oracle; the chaining values of column 0 of the 32764- and
    32765-row files at (1, 2) against read_ref.column_chunk_cvs (two columns of pure-Python BLAKE3)."""
    files = fleet(oracle, name)
    assert_one_group(pos, pos.ingest_plan([f.data.size for f in files], [f.pre for f in files], [f.enc for f in files]),
                     files)
    imgs = [np.full(f.enc * f.cap * 8, FILL, np.uint8) for f in files]
    res = pos.encode_files_grouped_into([f.data for f in files], [f.pre for f in files], [f.enc for f in files], imgs,
                                        [f.cap for f in files], True, True, True)
    for j, (f, o) in enumerate(zip(files, res)):
        at = (j, f.rows, f.pre, f.enc)
        assert o["rows_written"] == f.rows, at
        assert np.array_equal(imgs[j], f.img), at
        assert np.array_equal(o["tree"], f.tree), at
        assert o["root"] == f.root, at
        assert o["cvs"].shape == (read_ref.n_chunks(f.rows), f.enc, 32), at
        if f.pre == 1 and f.rows in (32764, 32765):
            want = read_ref.column_chunk_cvs([int(v) for v in f.elems[0, :f.rows]])
            got = [o["cvs"][c, 0].tobytes() for c in range(o["cvs"].shape[0])]
            assert got == [read_ref._words(w) for w in want], at


# ---------------------------------------------------------------- scrub and repair
def scrub(pos, files):
    return pos.scrub_files_grouped([f.img for f in files], [f.pre for f in files], [f.enc for f in files],
                                   [f.rows for f in files], [f.cap for f in files], [f.tree for f in files],
                                   [f.root for f in files], want_digests=True)


def assert_clean(r, f, at):
    assert not r["status"].any() and r["n_bad"] == 0 and r["n_dirty_rows"] == 0, at
    assert np.array_equal(r["digests"], f.tree[:f.enc]), at
    assert r["tree_consistent"] is True and r["root_ok"] is True, at


@pytest.mark.parametrize("name", list(FLEETS))
def test_scrub(pos, oracle, name):
    """A clean fleet scrubs clean with the oracle's leaves as digests; with the low bit of the last row of
    the last column flipped in every deep file, exactly that column of each is reported, one row is dirty,
    and the small files stay clean."""
    files = fleet(oracle, name)
    assert_one_group(pos, pos.scrub_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files]),
                     files)
    for j, (r, f) in enumerate(zip(scrub(pos, files), files)):
        assert_clean(r, f, j)
    bad = list(files)
    for j in deep_jobs(files):
        bad[j] = files[j].copy()
        bad[j].elems[-1, bad[j].rows - 1] ^= np.uint64(1)
        assert int(bad[j].elems[-1, bad[j].rows - 1]) < pos.FT63_MODULUS
    res = scrub(pos, bad)
    for j, (r, f) in enumerate(zip(res, files)):
        if j not in deep_jobs(files):
            assert_clean(r, f, j)
            continue
        assert list(np.flatnonzero(r["status"])) == [f.enc - 1] and r["status"][-1] == 1 and r["n_bad"] == 1, j
        assert r["n_dirty_rows"] == 1 and r["tree_consistent"] is True and r["root_ok"] is True, j
        assert np.array_equal(r["digests"][:-1], f.tree[:f.enc - 1]), j
        assert not np.array_equal(r["digests"][-1], f.tree[f.enc - 1]), j


@pytest.mark.parametrize("name", list(FLEETS))
def test_repair(pos, oracle, name):
    """The last column of every file overwritten with 0xFF words (slack included) and its stored leaf
    zeroed: the repaired column put back gives the oracle's image byte for byte, the digest is the oracle's
    leaf and the tree is the oracle's."""
    files = fleet(oracle, name)
    bads = [[f.enc - 1] for f in files]
    assert_one_group(pos, pos.repair_plan([f.rows for f in files], [f.pre for f in files], [f.enc for f in files],
                                     [1] * len(files)), files)
    damaged, leaves = [], []
    for f in files:
        g = f.copy()
        g.elems[-1, :] = FF
        lv = f.tree[:f.enc].copy()
        lv[-1] = 0
        damaged.append(g)
        leaves.append(lv)
    res = pos.repair_files_grouped([f.img for f in damaged], [f.pre for f in files], [f.enc for f in files],
                                   [f.rows for f in files], [f.cap for f in files], bads, leaves, want_tree=True)
    for j, (r, f, g) in enumerate(zip(res, files, damaged)):
        at = (j, f.rows, f.pre, f.enc)
        assert r["status"] == 0 and r["cols"].shape == (1, f.rows), at
        g.elems[-1, :f.rows] = r["cols"][0]
        g.elems[-1, f.rows:] = f.elems[-1, f.rows:]
        assert np.array_equal(g.img, f.img), at
        assert np.array_equal(r["digests"], f.tree[f.enc - 1:f.enc]), at
        assert np.array_equal(r["tree"], f.tree) and r["root"] == f.root, at


# ---------------------------------------------------------------- the grouped audit check
@pytest.fixture(scope="module")
def server(gpu, pos):
    return Server(gpu, pos)


def audits_of(gpu, server, rows_list, seed):
    """honest audits at (8, 16) with 1 and 5 opened columns per row count (the last column among the five),
    and two small jobs"""
    specs = [(r, n) for r in rows_list for n in (1, 5)] + [(3, 4), (253, 16)]
    rng = np.random.default_rng(seed)
    points = gpu.field_random(FT63, len(specs), seed)
    out = []
    for k, (rows, n_cols) in enumerate(specs):
        cols = sorted(rng.choice(15, size=n_cols - 1, replace=False).tolist()) + [15]
        out.append(server.audit(elems(rows, 8), 8, 16, rows % 5, points[k:k + 1], cols))
    return specs, out


def path_root(leaf, index, path, pyref):
    node = leaf
    for sibling in path:
        node = pyref.blake3(node + sibling if index % 2 == 0 else sibling + node)
        index >>= 1
    return node


@pytest.mark.parametrize("name", list(FLEETS))
def test_verify(gpu, pos, server, name):
    """Honest audits of files of the fleet's row counts, 1 and 5 opened columns each, plus two small jobs,
    in one pos.client_verify_evaluations_grouped call that the plan makes one grouped launch: verdicts and
    values equal the single check's job by job.  The leaf read_ref.leaf gives for the last opened column
    of the two deepest files leads to the root by the column's path (pure-Python BLAKE3: the leaf the
    grouped kernel accepted is that one).  With the low bit of the last element of the last opened column
    flipped in every deep job, each fails by its paths and the small jobs still pass."""
    import pyref
    rows_list = [r for r in DEEP_ROWS if name == "deep" or read_ref.n_chunks(r) <= 256]
    specs, audits = audits_of(gpu, server, rows_list, 40 + len(rows_list))
    tiles, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    assert launches == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any()
    assert set(tiles["job"].tolist()) == set(range(len(audits)))
    assert int(tiles["chunk"].max()) + 1 == read_ref.n_chunks(rows_list[-1])
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = pos.client_verify_evaluations_grouped(audits)
        _, count = gpu.prof_stats().get(VERIFY_REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert count == launches
    for j, a in enumerate(audits):
        want = single(gpu, pos, a)
        assert isinstance(want, np.ndarray), j
        same(gpu, got[j], want, f"job {j} {specs[j]}")
    for j in (2 * len(rows_list) - 3, 2 * len(rows_list) - 1):           # the five-column jobs of the two deepest files
        a = audits[j]
        column = a[7][-1]
        leaf = read_ref.leaf([read_ref.from_mont(v) for v in np.asarray(column.col).reshape(-1)])
        assert path_root(leaf, a[5][-1], list(column.path), pyref) == a[0], specs[j]
    bad = list(audits)
    for j in range(2 * len(rows_list)):
        col = audits[j][7][-1].col.copy()
        col.reshape(-1)[-1] ^= np.uint64(1)
        assert int(col.reshape(-1)[-1]) < read_ref.P
        bad[j] = with_column(audits[j], len(audits[j][7]) - 1, col=col)
    got = pos.client_verify_evaluations_grouped(bad)
    for j in range(len(bad)):
        if j < 2 * len(rows_list):
            assert isinstance(got[j], gpu.VerifierError) and names(got[j]) == "paths", (j, got[j])
        else:
            same(gpu, got[j], single(gpu, pos, audits[j]), f"job {j}")
    same(gpu, got[1], single(gpu, pos, bad[1]), "tampered job 1")
