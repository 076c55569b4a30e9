"""GPU: the batch and column-block seams of the stored-file host code, on files of a few KiB.

The stored-file paths stage an image through page-locked memory in row batches and column blocks of
256 MiB, so on every file a quick test can build they run as one batch and one block: the slot-reuse
wait, the partial last block and the partial last batch never execute.  LCPC_POS_STAGE_BYTES lowers
that budget.  At 7200 bytes a (16, 32) file of 301 rows goes through

* column blocks of 2 columns (7200 / (301 * 8)): 16 blocks, so both staging slots are reused;
* decode and re-encode batches of 28 rows (7200 / (32 * 8)): 11 batches, the last partial;
* writer, repair and locate batches of one BLAKE3 chunk (124 + 128 + 49 rows): 3 batches.

Shapes: (pre, enc) = (16, 32) and (2, 4); 125 rows (the first chunk's 124 rows and a one-row chunk)
and 301 rows (three chunks, the last of 49 rows: odd, so the cache's even-element pad is used); the
last row is short.

Every operation runs once with the knob unset and once at 7200, and each output is compared byte for
byte between the two; image and tree are also compared with the oracle's encode, the cache with the
writer's chaining values, the repaired columns and decoded bytes with the originals.  That the knob
acts at all is seen on the writer: one push of the whole 301-row file encodes rows before finalize
only when the batches are smaller than the file.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WB, DB = 8, 7
STAGE_BYTES = "7200"
DIMS = [(16, 32), (2, 4)]
ROWS = [125, 301]
CASES = [(pre, enc, rows) for pre, enc in DIMS for rows in ROWS]
EDIT_LO, EDIT_ROWS = 30, 60      # 60 rows from row 30: three 28-row batches, the last of 4 rows
APPEND_ROWS = 40
_runs = {}


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def _contents(pre, rows):
    n = rows * pre * DB - 3         # the last row is short
    return np.random.default_rng(97 * pre + rows).integers(0, 256, n, dtype=np.uint8).tobytes()


def _pick(enc, k, seed):
    return sorted(int(c) for c in np.random.default_rng(seed).permutation(enc)[:k])


def _columns(image, enc, cap):
    """a writable [enc][cap * 8] byte view of an image"""
    return image.reshape(enc, cap * WB)


def _run(PF, tmp_path, pre, enc, rows):
    """Every stored-file operation once on one file, under whatever the environment says: {name: bytes}."""
    from lcpc_proof_of_storage_amd import _native as N
    from lcpc_proof_of_storage_amd.lcpc2d import DeviceError, _raise
    lib, u8 = N.load(), PF._u8
    out = {}
    contents = _contents(pre, rows)
    data = np.frombuffer(contents, np.uint8)
    cap = 2 * rows
    rb = pre * DB

    # ---- the writer: image, tree, chunk chaining values; rows encoded before finalize
    img = np.zeros(enc * cap * WB, np.uint8)
    tree = np.zeros((2 * enc - 1) * 32, np.uint8)
    h = N.vp()
    _raise(lib.lcpc_pos_writer_new(pre, enc, u8(img), cap, 0, C.byref(h)))
    try:
        _raise(lib.lcpc_pos_writer_push_bytes(h, u8(data), data.size))
        out["rows_before_finalize"] = int(lib.lcpc_pos_writer_rows_written(h))
        n_rows = C.c_size_t()
        _raise(lib.lcpc_pos_writer_finalize(h, None, u8(tree), C.byref(n_rows), None))
        assert n_rows.value == rows
        cvs = PF._writer_chunk_cvs(h, enc)
    finally:
        lib.lcpc_pos_writer_free(h)
    out["image"], out["tree"], out["cvs"] = img.tobytes(), tree.tobytes(), cvs.tobytes()

    # ---- tree of the image
    t = np.zeros_like(tree)
    _raise(lib.lcpc_pos_porenc_tree(u8(img), enc, rows, cap, u8(t)))
    out["porenc_tree"] = t.tobytes()

    # ---- decode: every row, and a range that starts inside a batch of the full decode
    def decode(lo, hi):
        d = np.zeros((hi - lo) * rb, np.uint8)
        _raise(lib.lcpc_pos_decode_porenc(u8(img), pre, enc, cap, lo, hi, u8(d)))
        return d.tobytes()
    out["decode_all"] = decode(0, rows)
    out["decode_mid"] = decode(37, rows - 5)

    # ---- re-encode of rows in place, then the chunk cache after that edit
    edit = np.random.default_rng(rows + enc).integers(0, 256, EDIT_ROWS * rb, dtype=np.uint8)
    img2 = img.copy()
    _raise(lib.lcpc_pos_reencode_rows(u8(edit), edit.size, pre, enc, EDIT_LO, u8(img2), cap))
    out["reencode_image"] = img2.tobytes()

    cache = PF.ColumnChunkCache.from_porenc(img, enc, rows, cap)
    out["cache_cvs"] = cache.copy_cvs().tobytes()
    cache.update(img2, cap, EDIT_LO, EDIT_LO + EDIT_ROWS, rows)
    out["cache_edit_map"] = cache.copy_cvs().tobytes()
    path = tmp_path / "image.porenc"
    path.write_bytes(img2.tobytes())
    cache_fd = PF.ColumnChunkCache.from_cvs(cvs, enc, rows)
    with open(path, "rb") as f:
        cache_fd.update_file(f, cap, EDIT_LO, EDIT_LO + EDIT_ROWS, rows)
    out["cache_edit_fd"] = cache_fd.copy_cvs().tobytes()

    # ---- append: new rows after the last, then both caches again
    more = np.random.default_rng(rows + pre).integers(0, 256, APPEND_ROWS * rb, dtype=np.uint8)
    img3 = img2.copy()
    _raise(lib.lcpc_pos_reencode_rows(u8(more), more.size, pre, enc, rows, u8(img3), cap))
    new_rows = rows + APPEND_ROWS
    cache.update(img3, cap, rows, new_rows, new_rows)
    out["cache_append_map"] = cache.copy_cvs().tobytes()
    path.write_bytes(img3.tobytes())
    with open(path, "rb") as f:
        cache_fd.update_file(f, cap, rows, new_rows, new_rows)
    out["cache_append_fd"] = cache_fd.copy_cvs().tobytes()
    fresh = PF.ColumnChunkCache.from_porenc(img3, enc, new_rows, cap)
    out["cache_append_fresh"] = fresh.copy_cvs().tobytes()
    for c in (cache, cache_fd, fresh):
        c.close()

    # ---- scrub: one flipped bit in the last column (a late block), one column of 0xFF
    img_s = img.copy()
    _columns(img_s, enc, cap)[enc - 1, (rows - 1) * WB + 2] ^= 0x08
    _columns(img_s, enc, cap)[1, :rows * WB] = 0xFF
    status, digests, n_bad = np.zeros(enc, np.uint8), np.zeros(enc * 32, np.uint8), C.c_size_t()
    _raise(lib.lcpc_pos_scrub_porenc(u8(img_s), enc, rows, cap, u8(tree[:enc * 32]), u8(digests), u8(status),
                                     C.byref(n_bad)))
    assert n_bad.value == 2
    out["scrub_status"], out["scrub_digests"] = status.tobytes(), digests.tobytes()

    # ---- locate: the 0xFF column makes the first pass void; the image is scanned and a second pass run
    img_l = img.copy()
    _columns(img_l, enc, cap)[1, :rows * WB] = 0xFF
    col_status = np.zeros(enc, np.uint8)
    counts = [C.c_size_t() for _ in range(3)]
    _raise(lib.lcpc_pos_locate_porenc(u8(img_l), pre, enc, rows, cap, None, 0, u8(col_status),
                                      *[C.byref(x) for x in counts]))
    out["locate_status"] = col_status.tobytes()
    out["locate_counts"] = bytes(str([x.value for x in counts]), "ascii")

    # ---- repair of enc - pre columns, with the data out
    cols = _pick(enc, enc - pre, rows + enc)
    img_r = img.copy()
    for c in cols:
        _columns(img_r, enc, cap)[c, :rows * WB] = 0xFF
    idx = np.asarray(cols, np.uint64)
    got = np.zeros(len(cols) * rows * WB, np.uint8)
    dig = np.zeros(len(cols) * 32, np.uint8)
    dat = np.zeros(rows * rb, np.uint8)
    _raise(lib.lcpc_pos_repair_columns(u8(img_r), pre, enc, rows, cap, idx.ctypes.data_as(N.u64p), len(cols),
                                       u8(got), u8(dig), u8(dat)))
    out["repair_cols"], out["repair_digests"], out["repair_data"] = got.tobytes(), dig.tobytes(), dat.tobytes()
    out["repair_want_cols"] = _columns(img, enc, cap)[cols, :rows * WB].tobytes()
    out["repair_want_digests"] = b"".join(tree[32 * c:32 * c + 32].tobytes() for c in cols)

    # ---- the tree call's error for a non-canonical element in the last block
    img_e = img.copy()
    _columns(img_e, enc, cap)[enc - 1, (rows - 1) * WB:rows * WB] = 0xFF
    with pytest.raises(DeviceError) as err:
        _raise(lib.lcpc_pos_porenc_tree(u8(img_e), enc, rows, cap, u8(t)))
    out["tree_error"] = str(err.value).encode()
    return out


def _both(PF, monkeypatch, tmp_path_factory, pre, enc, rows):
    """(outputs with the knob unset, outputs at 7200 bytes), computed once per shape"""
    key = (pre, enc, rows)
    if key not in _runs:
        monkeypatch.delenv("LCPC_POS_STAGE_BYTES", raising=False)
        plain = _run(PF, tmp_path_factory.mktemp(f"plain_{pre}_{enc}_{rows}"), pre, enc, rows)
        monkeypatch.setenv("LCPC_POS_STAGE_BYTES", STAGE_BYTES)
        small = _run(PF, tmp_path_factory.mktemp(f"small_{pre}_{enc}_{rows}"), pre, enc, rows)
        _runs[key] = (plain, small)
    return _runs[key]


OPS = ["image", "tree", "cvs", "porenc_tree", "decode_all", "decode_mid", "reencode_image", "cache_cvs",
       "cache_edit_map", "cache_edit_fd", "cache_append_map", "cache_append_fd", "cache_append_fresh",
       "scrub_status", "scrub_digests", "locate_status", "locate_counts", "repair_cols", "repair_digests",
       "repair_data", "tree_error"]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_small_batches_give_the_same_bytes(PF, monkeypatch, tmp_path_factory, pre, enc, rows, op):
    plain, small = _both(PF, monkeypatch, tmp_path_factory, pre, enc, rows)
    assert plain[op] == small[op]


@pytest.mark.parametrize("knob", [0, 1])
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_outputs_are_the_right_ones(PF, oracle, monkeypatch, tmp_path_factory, pre, enc, rows, knob):
    """not merely equal to each other: against the oracle, the writer and the undamaged file"""
    o = _both(PF, monkeypatch, tmp_path_factory, pre, enc, rows)[knob]
    contents = _contents(pre, rows)
    img, otree, orows, ocap = oracle.pos_encode_file(contents, pre, enc)
    assert (orows, ocap) == (rows, 2 * rows)
    assert o["image"] == bytes(img) and o["tree"] == bytes(otree) and o["porenc_tree"] == bytes(otree)
    padded = contents + bytes(rows * pre * DB - len(contents))
    assert o["decode_all"] == padded and o["decode_mid"] == padded[37 * pre * DB:(rows - 5) * pre * DB]
    assert o["cache_cvs"] == o["cvs"]
    assert o["cache_edit_map"] == o["cache_edit_fd"] != o["cvs"]
    assert o["cache_append_map"] == o["cache_append_fd"] == o["cache_append_fresh"]
    status = np.frombuffer(o["scrub_status"], np.uint8)
    assert [int(c) for c in np.flatnonzero(status)] == [1, enc - 1] and status[1] == 2 and status[enc - 1] == 1
    lstatus = np.frombuffer(o["locate_status"], np.uint8)
    assert [int(c) for c in np.flatnonzero(lstatus)] == [1] and lstatus[1] == 2
    assert o["repair_cols"] == o["repair_want_cols"] and o["repair_digests"] == o["repair_want_digests"]
    assert o["repair_data"] == padded
    assert b"from_repr fails" in o["tree_error"]
    # the edited rows decode to the edit: the re-encode wrote the right rows, and only those
    a = np.frombuffer(o["image"], np.uint8).reshape(enc, 2 * rows * WB)
    b = np.frombuffer(o["reencode_image"], np.uint8).reshape(enc, 2 * rows * WB)
    same = np.ones(2 * rows * WB, bool)
    same[EDIT_LO * WB:(EDIT_LO + EDIT_ROWS) * WB] = False
    assert np.array_equal(a[:, same], b[:, same]) and not np.array_equal(a, b)


def test_the_knob_is_seen_to_act(PF, monkeypatch, tmp_path_factory):
    """One push of the whole 301-row file: with one-chunk batches the writer encodes the chunks the
    data provably continues past at once; with the default budget the file is less than a batch and
    every row waits for finalize."""
    plain, small = _both(PF, monkeypatch, tmp_path_factory, 16, 32, 301)
    assert plain["rows_before_finalize"] == 0
    assert small["rows_before_finalize"] > 0
