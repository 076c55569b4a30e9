"""GPU: scrub and repair of stored proof-of-storage files (FileHandler.scrub / repair,
EncodedFileReader.find_damaged_columns / repair_columns / decode_with_erasures over
lcpc_pos_scrub_porenc and lcpc_pos_repair_columns; no counterpart in the reference).

Files are built with FileHandler.create_from_unencoded_file and checked against the oracle's
encode, dims (2,4) and (16,32), 1 / 124 / 125 / 300 rows (either side of the first BLAKE3 chunk
boundary of a column message, at row 124).  Then they are damaged:

* one flipped bit; a whole column of 0xFF (non-canonical: status 2); enc - pre damaged columns;
* bytes in the slack rows past rows_written (scrub: clean);
* one damaged `.portree` leaf (repaired only with expected_root);
* a damaged raw file;
* enc - pre + 1 columns with a sound raw file (the re-encode fallback);
* enc - pre + 1 columns and a damaged raw file: UnrecoverableError, every file byte-identical;
* a wrong expected_root: refused, every file byte-identical.

After every successful repair the written rows of every `.porenc` column equal the pre-damage
image, the tree file is unchanged, verify_all_files_agree passes and a second scrub is clean;
decode_with_erasures gave the original bytes from the damaged file before anything was written.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WB = 8
DIMS = [(2, 4), (16, 32)]
ROWS = [1, 124, 125, 300]
CASES = [(pre, enc, rows) for pre, enc in DIMS for rows in ROWS]
ULID = "01REPAIRTEST00000000000000"
EXTS = ("porraw", "porenc", "portree", "meta")
_pristine = {}


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _contents(pre, rows):
    n = rows * pre * 7 - 3          # the last row is short
    return np.random.default_rng(97 * pre + rows).integers(0, 256, n, dtype=np.uint8).tobytes()


def pristine(PF, oracle, tmp_path_factory, pre, enc, rows):
    """The four files of a fresh store, checked against the oracle once per shape: {ext: bytes}."""
    key = (pre, enc, rows)
    if key not in _pristine:
        d = tmp_path_factory.mktemp(f"pristine_{pre}_{enc}_{rows}")
        contents = _contents(pre, rows)
        src = d / "in.bin"
        src.write_bytes(contents)
        fh = PF.FileHandler.create_from_unencoded_file(ULID, str(src), pre, enc, directory=str(d / "store"))
        img, otree, orows, ocap = oracle.pos_encode_file(contents, pre, enc)
        assert (orows, ocap) == (rows, fh.row_capacity) and fh.rows_written == rows
        files = {e: _read(d / "store" / f"{ULID}.{e}") for e in EXTS}
        assert len(files["porenc"]) == len(img)
        assert np.array_equal(written(files["porenc"], enc, ocap, rows), written(img, enc, ocap, rows))
        assert files["portree"] == otree and files["porraw"] == contents
        _pristine[key] = files
    return _pristine[key]


def store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows, chunk_cache=False):
    """A private copy of the pristine files and a handler attached to it."""
    files = pristine(PF, oracle, tmp_path_factory, pre, enc, rows)
    d = tmp_path / "store"
    d.mkdir()
    for e, b in files.items():
        (d / f"{ULID}.{e}").write_bytes(b)
    return PF.FileHandler.new_attach_to_existing_ulid(str(d), ULID, chunk_cache=chunk_cache), files


def snapshot(fh):
    return {e: _read(os.path.join(os.path.dirname(fh.get_encoded_file_handle()), f"{ULID}.{e}")) for e in EXTS}


def poke(path, offset, data):
    with open(path, "r+b") as f:
        f.seek(offset)
        f.write(data)


def damage_columns(fh, cols, seed, ff=False):
    """rows_written elements of each listed column replaced (random bytes, or 0xFF)"""
    rng = np.random.default_rng(seed)
    n = fh.rows_written * WB
    for c in cols:
        junk = b"\xff" * n if ff else rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        poke(fh.get_encoded_file_handle(), c * fh.row_capacity * WB, junk)


def written(image, enc, cap, rows):
    return np.frombuffer(image, np.uint8).reshape(enc, cap * WB)[:, :rows * WB]


def decode_from_damaged(PF, fh, cols):
    with open(fh.get_encoded_file_handle(), "rb") as f:
        r = PF.EncodedFileReader.new_ligero(f, fh.pre_encoded_size, fh.encoded_size, fh.rows_written, fh.row_capacity)
        return r.decode_with_erasures(cols)


def check_repaired(fh, files):
    pre, enc, rows = fh.get_dimensions()
    now = snapshot(fh)
    assert np.array_equal(written(now["porenc"], enc, fh.row_capacity, rows),
                          written(files["porenc"], enc, fh.row_capacity, rows))
    assert now["portree"] == files["portree"]
    assert now["porraw"] == files["porraw"]
    fh.verify_all_files_agree()
    again = fh.scrub()
    assert again.clean and again.bad_columns == [] and again.tree_consistent and again.raw_ok


def pick(enc, k, seed):
    return sorted(int(c) for c in np.random.default_rng(seed).permutation(enc)[:k])


# ---------------------------------------------------------------- a sound store
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_sound_store_is_clean_and_repair_writes_nothing(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    root = fh.get_commit_root()
    rep = fh.scrub(expected_root=root)
    assert rep.clean and rep.root_ok is True and rep.noncanonical_columns == []
    assert fh.scrub().root_ok is None
    assert fh.repair().repaired_from is None and snapshot(fh) == files
    # the reader's pieces: nothing damaged, any enc - pre columns are recomputed as they are
    cols = pick(enc, enc - pre, rows)
    with open(fh.get_encoded_file_handle(), "rb") as f:
        r = PF.EncodedFileReader.new_ligero(f, pre, enc, rows, fh.row_capacity)
        assert r.find_damaged_columns(fh.get_merkle_tree()) == ([], [])
        got, dig = r.repair_columns(cols)
        assert r.decode_with_erasures([])[:len(files["porraw"])] == files["porraw"]
    want = np.frombuffer(files["porenc"], "<u8").reshape(enc, fh.row_capacity)[cols, :rows]
    assert np.array_equal(got, want)
    assert [d.tobytes() for d in dig] == [fh.get_merkle_tree()[c] for c in cols]


# ---------------------------------------------------------------- damaged columns
@pytest.mark.parametrize("kind", ["bit", "ff", "max"])
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_damaged_columns_are_located_and_recomputed(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows, kind):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    if kind == "bit":
        cols = [enc - 1]
        off = (cols[0] * fh.row_capacity + rows - 1) * WB + 2
        poke(fh.get_encoded_file_handle(), off, bytes([files["porenc"][off] ^ 0x08]))
    elif kind == "ff":
        cols = [1]
        damage_columns(fh, cols, 0, ff=True)
    else:
        cols = pick(enc, enc - pre, 7 * rows + enc)
        damage_columns(fh, cols, rows)
    rep = fh.scrub()
    assert rep.bad_columns == cols and rep.tree_consistent and rep.raw_ok and not rep.clean
    assert rep.noncanonical_columns == (cols if kind == "ff" else rep.noncanonical_columns)
    assert set(rep.noncanonical_columns) <= set(cols)
    from lcpc_proof_of_storage_amd import lcpc2d
    # (what there was before: "trees differ", or a failed call on a non-canonical element)
    with pytest.raises((AssertionError, lcpc2d.DeviceError)):
        fh.verify_all_files_agree()
    # the download path: the original bytes from the damaged replica, nothing written
    before = snapshot(fh)
    assert decode_from_damaged(PF, fh, cols)[:len(files["porraw"])] == files["porraw"]
    assert snapshot(fh) == before
    done = fh.repair()
    assert done.bad_columns == cols and done.repaired_from == "columns"
    check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_slack_rows_are_not_looked_at(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    assert fh.row_capacity > rows
    for c in (0, enc - 1):
        poke(fh.get_encoded_file_handle(), (c * fh.row_capacity + rows) * WB, b"\xff" * WB)
    assert fh.scrub().clean
    assert fh.repair().repaired_from is None
    check_repaired(fh, files)


# ---------------------------------------------------------------- the tree and the raw file
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_damaged_leaf_needs_the_expected_root(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    root = fh.get_commit_root()
    c = enc // 2
    poke(fh.get_merkle_file_handle(), 32 * c + 5, bytes([files["portree"][32 * c + 5] ^ 0x40]))
    before = snapshot(fh)
    rep = fh.scrub(expected_root=root)
    assert rep.bad_columns == [c] and not rep.tree_consistent and rep.root_ok is True and not rep.raw_ok
    with pytest.raises(PF.UnrecoverableError):      # the stored tree does not refold: no anchor of its own
        fh.repair()
    assert snapshot(fh) == before
    done = fh.repair(expected_root=root)
    assert done.repaired_from == "tree"
    check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_damaged_raw_file_is_rewritten_from_the_decode(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    off = len(files["porraw"]) // 2
    poke(fh.get_raw_file_handle(), off, bytes([files["porraw"][off] ^ 0x01]))
    rep = fh.scrub()
    assert rep.bad_columns == [] and rep.tree_consistent and not rep.raw_ok
    assert fh.repair().repaired_from == "raw"
    check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_columns_and_raw_file_damaged_together(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    cols = pick(enc, enc - pre, rows + 1)
    damage_columns(fh, cols, 3)
    poke(fh.get_raw_file_handle(), 0, bytes([files["porraw"][0] ^ 0x80]))
    assert fh.repair(expected_root=fh.get_commit_root()).repaired_from == "columns+raw"
    check_repaired(fh, files)


# ---------------------------------------------------------------- beyond the code's redundancy
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_too_many_columns_fall_back_to_the_raw_file(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    cols = pick(enc, enc - pre + 1, rows + 2)
    damage_columns(fh, cols, 4)
    rep = fh.scrub()
    assert rep.bad_columns == cols and rep.raw_ok
    with pytest.raises(PF.UnrecoverableError):
        decode_from_damaged(PF, fh, cols)
    assert fh.repair().repaired_from == "reencode"
    check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_unrecoverable_leaves_every_file_as_it_was(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    damage_columns(fh, pick(enc, enc - pre + 1, rows + 3), 5)
    poke(fh.get_raw_file_handle(), len(files["porraw"]) - 1, bytes([files["porraw"][-1] ^ 0x10]))
    before = snapshot(fh)
    for root in (None, fh.get_commit_root()):
        with pytest.raises(PF.UnrecoverableError):
            fh.repair(expected_root=root)
        assert snapshot(fh) == before


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_wrong_expected_root_is_refused(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    wrong = bytes(b ^ 0xA5 for b in fh.get_commit_root())
    assert fh.scrub(expected_root=wrong).root_ok is False and not fh.scrub(expected_root=wrong).clean
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(expected_root=wrong)
    assert snapshot(fh) == files
    damage_columns(fh, [0], 6)                      # mendable damage, but nothing verifies against that root
    before = snapshot(fh)
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(expected_root=wrong)
    assert snapshot(fh) == before
    assert fh.repair().repaired_from == "columns"
    check_repaired(fh, files)


# ---------------------------------------------------------------- row batches
@pytest.mark.parametrize("batch_rows", [1, 128, 256])
@pytest.mark.parametrize("pre,enc", DIMS)
def test_row_batches_end_on_chunk_boundaries(PF, oracle, tmp_path_factory, tmp_path, monkeypatch, pre, enc, batch_rows):
    """300 rows are three column chunks (124 + 128 + 48 rows): one chunk per batch (three batches,
    a request for less than a chunk included) and two per batch give the columns, the digests folded
    from the batches' chaining values and the decode of one batch"""
    rows = 300
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    cols = pick(enc, enc - pre, batch_rows)
    damage_columns(fh, cols, 9, ff=True)
    monkeypatch.setenv("LCPC_POS_REPAIR_BATCH_ROWS", str(batch_rows))
    with open(fh.get_encoded_file_handle(), "rb") as f:
        r = PF.EncodedFileReader.new_ligero(f, pre, enc, rows, fh.row_capacity)
        got, dig = r.repair_columns(cols)
        data = r.decode_with_erasures(cols)
    want = np.frombuffer(files["porenc"], "<u8").reshape(enc, fh.row_capacity)[cols, :rows]
    assert np.array_equal(got, want)
    assert [d.tobytes() for d in dig] == [fh.get_merkle_tree()[c] for c in cols]
    assert data[:len(files["porraw"])] == files["porraw"]
    assert fh.repair().repaired_from == "columns"
    check_repaired(fh, files)


# ---------------------------------------------------------------- with the chunk-CV cache
def test_repair_rebuilds_the_chunk_cache_and_its_sidecar(PF, oracle, tmp_path_factory, tmp_path):
    pre, enc, rows = 16, 32, 300
    fh, files = store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows, chunk_cache=True)
    cols = pick(enc, 5, 11)
    damage_columns(fh, cols, 8)
    assert fh.repair().repaired_from == "columns"
    check_repaired(fh, files)                       # (verify_all_files_agree compares with a rebuilt cache)
    data = _read(fh.chunk_cv_file_handle)
    n = PF.check_chunk_cv_sidecar(data[:64], len(data), enc, rows, fh.get_merkle_tree().root())
    assert n == fh.chunk_cache.n_chunks
    fresh = fh._rebuild_chunk_cache()
    try:
        assert data[64:64 + n * enc * 32] == fresh.copy_cvs().tobytes() == fh.chunk_cache.copy_cvs().tobytes()
    finally:
        fresh.close()
