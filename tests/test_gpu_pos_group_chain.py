"""GPU: the three grouped entries of stored files one after another in one process -- grouped ingest,
grouped scrub of what it made, grouped repair of one erased column per file, then the three again in
reverse order.  They share one twiddle table per device and one two-slot staging pipeline:
a table built wrong for the entry that did not build it, or a slot handed to its jobs in the wrong order,
shows here.  LCPC_POS_GROUP_BYTES = 4096 cuts the five files into at least three groups per entry, so
both slots are reused; the file of 2048 points takes the single-file path and, in scrub and repair, its
tree-only group through the same slots.  Every output is compared with the single-file entries
(lcpc_pos_encode_file, lcpc_pos_scrub_porenc, lcpc_pos_locate_porenc, lcpc_pos_repair_columns), exactly."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
# (pre, enc, rows): ingest groups {0}, {1, 2}, {4} and file 3 alone; scrub and repair route file 0 (its
# packed image is above the group) and file 3 to the single-file entries and group {1, 2} and {4}
FILES = [(63, 64, 9), (63, 64, 1), (1, 2, 9), (1024, 2048, 1), (512, 1024, 0)]
BAD = [5, 63, 1, 2047, 0]   # the erased column of each file


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


@pytest.fixture(scope="module")
def single(native):
    """per file what the single-file entries give: data, image (enc, rows), tree, scrub status / digests /
    n_bad / dirty rows of the damaged image, and the repaired column and digest"""
    lib, out = native.load(), []
    for j, (pre, enc, rows) in enumerate(FILES):
        data = np.random.default_rng(100 + j).integers(0, 256, max(rows * 7 * pre - 2, 0), dtype=np.uint8)
        img, tree, got = np.zeros((enc, rows), np.uint64), np.zeros((2 * enc - 1, 32), np.uint8), C.c_size_t()
        assert lib.lcpc_pos_encode_file(u8(data), data.size, pre, enc, rows, u8(img.view(np.uint8).reshape(-1)),
                                        u8(tree.reshape(-1)), C.byref(got)) == 0
        assert got.value == rows
        hurt = img.copy()
        hurt[BAD[j], :] = FF
        status, digests, n_bad = np.zeros(enc, np.uint8), np.zeros((enc, 32), np.uint8), C.c_size_t()
        assert lib.lcpc_pos_scrub_porenc(u8(img.view(np.uint8).reshape(-1)), enc, rows, rows, u8(tree[:enc].reshape(-1)),
                                         u8(digests.reshape(-1)), u8(status), C.byref(n_bad)) == 0
        located, nb, nd, nu = np.zeros(enc, np.uint8), C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert lib.lcpc_pos_locate_porenc(u8(img.view(np.uint8).reshape(-1)), pre, enc, rows, rows, None, 0, u8(located),
                                          C.byref(nb), C.byref(nd), C.byref(nu)) == 0
        bad = np.array([BAD[j]], np.uint64)
        col, dig = np.zeros((1, rows), np.uint64), np.zeros((1, 32), np.uint8)
        assert lib.lcpc_pos_repair_columns(u8(hurt.view(np.uint8).reshape(-1)), pre, enc, rows, rows,
                                           bad.ctypes.data_as(C.POINTER(C.c_uint64)), 1,
                                           u8(col.view(np.uint8).reshape(-1)), u8(dig.reshape(-1)), None) == 0
        out.append(dict(data=data, img=img, tree=tree, hurt=hurt, status=status, digests=digests, n_bad=n_bad.value,
                        n_dirty=nd.value, col=col, dig=dig))
    return out


def ingest(pos, single):
    res = pos.encode_files_grouped([s["data"] for s in single], [f[0] for f in FILES], [f[1] for f in FILES])
    for j, ((img, tree, rows), s) in enumerate(zip(res, single)):
        assert rows == FILES[j][2], j
        assert np.array_equal(img, s["img"]), j
        assert np.array_equal(tree, s["tree"]), j


def scrub(pos, single):
    res = pos.scrub_files_grouped([s["img"] for s in single], [f[0] for f in FILES], [f[1] for f in FILES],
                                  [f[2] for f in FILES], [f[2] for f in FILES], [s["tree"] for s in single],
                                  [s["tree"][-1].tobytes() for s in single], want_digests=True)
    for j, (r, s) in enumerate(zip(res, single)):
        assert np.array_equal(r["status"], s["status"]) and not r["status"].any(), j
        assert np.array_equal(r["digests"], s["digests"]) and np.array_equal(r["digests"], s["tree"][:FILES[j][1]]), j
        assert r["n_bad"] == s["n_bad"] == 0 and r["n_dirty_rows"] == s["n_dirty"] == 0, j
        assert r["tree_consistent"] is True and r["root_ok"] is True, j


def repair(pos, single):
    leaves = []
    for j, s in enumerate(single):
        lv = s["tree"][:FILES[j][1]].copy()
        lv[BAD[j]] = 0                      # the stale leaf of the erased column: the repaired digest replaces it
        leaves.append(lv)
    res = pos.repair_files_grouped([s["hurt"] for s in single], [f[0] for f in FILES], [f[1] for f in FILES],
                                   [f[2] for f in FILES], [f[2] for f in FILES], [[b] for b in BAD], leaves,
                                   want_cols=True, want_tree=True)
    for j, (r, s) in enumerate(zip(res, single)):
        assert r["status"] == 0, j
        assert np.array_equal(r["cols"], s["col"]) and np.array_equal(r["cols"][0], s["img"][BAD[j]]), j
        assert np.array_equal(r["digests"], s["dig"]) and np.array_equal(r["digests"][0], s["tree"][BAD[j]]), j
        assert np.array_equal(r["tree"], s["tree"]) and r["root"] == s["tree"][-1].tobytes(), j


def test_ingest_scrub_repair_and_back_share_the_table_and_the_slots(pos, single, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", "4096")
    pres, encs, rows = [f[0] for f in FILES], [f[1] for f in FILES], [f[2] for f in FILES]
    tiles, n_groups = pos.ingest_plan([s["data"].size for s in single], pres, encs)
    assert n_groups >= 3 and list(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE]) == [3]
    tiles, n_groups = pos.scrub_plan(rows, pres, encs)
    assert n_groups == 2 and list(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE]) == [0, 3]   # + 2 tree-only groups
    tiles, n_groups = pos.repair_plan(rows, pres, encs, [1] * len(FILES))
    assert n_groups == 2 and list(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE]) == [0, 3]
    for step in (ingest, scrub, repair, repair, scrub, ingest):
        step(pos, single)
