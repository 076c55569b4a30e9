"""GPU: damaged `.porenc` columns located without a tree (EncodedFileReader.locate_damaged_columns over
lcpc_pos_locate_porenc; FileHandler.scrub / repair with locate=True; no counterpart in the reference).

Files as tests/test_gpu_pos_repair.py builds them (its helpers and its cache of pristine stores are
shared): dims (2,4) and (16,32), 1 / 124 / 125 / 300 rows.  Damage: one low bit of one element; an
all-ones word (not < p: status 2); a byte run in one column across the chunk seam at row 124; a whole
column of wrong canonical elements; a whole column of random bytes (status 2 once an element is not
< p); (enc - pre) / 2 whole canonical columns (every row at its radius); a column listed as known
(status 3, never read).  Also with LCPC_POS_REPAIR_BATCH_ROWS=128 and dirty rows on
both sides of both batch seams of a 300-row file.

* locate_damaged_columns names exactly the damaged columns with their status codes;
* scrub(locate=True) on a clean file reports [] and 0; with a sound tree located_columns ==
  bad_columns (the two locators check each other);
* repair(locate=True) restores `.porenc` rows, tree and raw file byte for byte, then
  verify_all_files_agree and a clean second scrub: tree file deleted + element damage + expected_root;
  tree file truncated + no root + sound raw file; more than enc - pre leaves overwritten + `.porenc`
  damage + damaged raw file + expected_root;
* UnrecoverableError with all four files byte-identical: tree missing + no root + damaged raw file;
  one row with more wrong elements than its radius + a bad raw file; a wrong expected_root.
"""
import os

import numpy as np
import pytest

import test_gpu_pos_repair as T

pytestmark = pytest.mark.gpu
WB = T.WB
CASES = T.CASES
KINDS = ["bit", "ones", "run", "col", "rawcol", "half"]


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def canonical_junk(oracle, n, seed):
    """n wrong elements that are < p, as file bytes"""
    p = oracle.modulus(0)
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 1 << 62, n, dtype=np.uint64) % np.uint64(p)).astype("<u8").tobytes()


def junk_columns(oracle, fh, cols, seed):
    for k, c in enumerate(cols):
        T.poke(fh.get_encoded_file_handle(), c * fh.row_capacity * WB,
               canonical_junk(oracle, fh.rows_written, seed + k))


def flip_low_bit(fh, files, col, row):
    off = (col * fh.row_capacity + row) * WB
    T.poke(fh.get_encoded_file_handle(), off, bytes([files["porenc"][off] ^ 0x01]))


def apply_damage(oracle, fh, files, kind, pre, enc, rows):
    """{column: status} of what was damaged"""
    if kind == "bit":
        flip_low_bit(fh, files, enc - 1, rows - 1)
        return {enc - 1: 1}
    if kind == "ones":
        T.poke(fh.get_encoded_file_handle(), (1 * fh.row_capacity + rows // 2) * WB, b"\xff" * WB)
        return {1: 2}
    if kind == "run":
        lo, hi = max(0, min(rows, 124) - 3), min(rows, 127)       # rows on both sides of the seam, where there are
        off = (2 * fh.row_capacity + lo) * WB
        old = files["porenc"][off:off + (hi - lo) * WB]
        new = bytes(b ^ (0x5A if i % WB < 7 else 0) for i, b in enumerate(old))   # top bytes kept: still < p
        assert all(int.from_bytes(new[i:i + WB], "little") < oracle.modulus(0) for i in range(0, len(new), WB))
        T.poke(fh.get_encoded_file_handle(), off, new)
        return {2: 1}
    if kind == "rawcol":      # a whole column of random bytes: status 2 as soon as one element is not < p
        T.damage_columns(fh, [enc - 1], 17 * rows + enc)
        with open(fh.get_encoded_file_handle(), "rb") as f:
            f.seek((enc - 1) * fh.row_capacity * WB)
            now = np.frombuffer(f.read(rows * WB), "<u8")
        return {enc - 1: 2 if any(int(v) >= oracle.modulus(0) for v in now) else 1}
    cols = [0] if kind == "col" else T.pick(enc, (enc - pre) // 2, 5 * rows + enc)
    junk_columns(oracle, fh, cols, 31 * rows + enc)
    # (a junk element equals the stored one with probability 2^-62)
    return {c: 1 for c in cols}


def locate(PF, fh, known=()):
    with open(fh.get_encoded_file_handle(), "rb") as f:
        r = PF.EncodedFileReader.new_ligero(f, fh.pre_encoded_size, fh.encoded_size, fh.rows_written, fh.row_capacity)
        return r.locate_damaged_columns(known)


# ---------------------------------------------------------------- locating
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_clean_file_has_nothing_to_locate(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    status, unloc = locate(PF, fh)
    assert not status.any() and unloc == 0
    rep = fh.scrub(locate=True)
    assert rep.located_columns == [] and rep.unlocatable_rows == 0 and rep.clean
    plain = fh.scrub()
    assert plain.located_columns is None and plain.unlocatable_rows is None
    assert fh.repair(locate=True).repaired_from is None and T.snapshot(fh) == files


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_damaged_columns_are_named_with_their_status(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows, kind):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    want = apply_damage(oracle, fh, files, kind, pre, enc, rows)
    before = T.snapshot(fh)
    status, unloc = locate(PF, fh)
    assert {int(c): int(status[c]) for c in np.flatnonzero(status)} == want and unloc == 0
    rep = fh.scrub(locate=True)                     # the tree is sound: the two locators agree
    assert rep.located_columns == rep.bad_columns == sorted(want) and rep.unlocatable_rows == 0
    assert rep.noncanonical_columns == [c for c in sorted(want) if want[c] == 2]
    assert T.snapshot(fh) == before


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_known_columns_are_never_read(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    T.damage_columns(fh, [enc - 2], 3, ff=True)     # non-canonical, but listed: status 3, not 2
    flip_low_bit(fh, files, 0, 0)
    status, unloc = locate(PF, fh, known=[enc - 2])
    if enc - pre - 1 >= 2:
        assert {int(c): int(status[c]) for c in np.flatnonzero(status)} == {0: 1, enc - 2: 3} and unloc == 0
    else:   # (2,4): one erasure leaves one syndrome -- an error is seen but cannot be located
        assert {int(c): int(status[c]) for c in np.flatnonzero(status)} == {enc - 2: 3} and unloc == 1
    # all of the redundancy listed: no syndromes are left, every row passes
    known = list(range(pre, enc))
    status, unloc = locate(PF, fh, known=known)
    assert [int(c) for c in np.flatnonzero(status)] == known and set(status[known]) == {3} and unloc == 0
    T.damage_columns(fh, [0], 4, ff=True)
    with pytest.raises(PF.UnrecoverableError):      # more known and non-canonical columns than the code can spare
        locate(PF, fh, known=[c for c in known if c != enc - 2] + [1])


@pytest.mark.parametrize("pre,enc", T.DIMS)
def test_dirty_rows_on_both_sides_of_the_batch_seams(PF, oracle, tmp_path_factory, tmp_path, monkeypatch, pre, enc):
    """300 rows are three column chunks (124 + 128 + 48 rows); one chunk per batch"""
    rows = 300
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    monkeypatch.setenv("LCPC_POS_REPAIR_BATCH_ROWS", "128")
    hits = {123: 0, 124: 1, 251: 0, 252: 2, 299: 1}
    for row, col in hits.items():
        flip_low_bit(fh, files, col, row)
    T.poke(fh.get_encoded_file_handle(), (3 * fh.row_capacity + 200) * WB, b"\xff" * WB)
    status, unloc = locate(PF, fh)
    want = {c: 1 for c in hits.values()}
    want[3] = 2
    if enc - pre - 1 < 2:       # (2,4) with column 3 an erasure: the other errors are seen, not located
        assert {int(c): int(status[c]) for c in np.flatnonzero(status)} == {3: 2} and unloc == len(hits)
        return
    assert {int(c): int(status[c]) for c in np.flatnonzero(status)} == want and unloc == 0
    done = fh.repair(locate=True)                   # the tree is sound: the existing path mends it
    assert done.repaired_from == "columns"
    T.check_repaired(fh, files)


# ---------------------------------------------------------------- repair where the tree cannot help
def damage_raw(fh, files):
    off = len(files["porraw"]) // 3
    T.poke(fh.get_raw_file_handle(), off, bytes([files["porraw"][off] ^ 0x04]))


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_repair_with_the_tree_file_deleted(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    root = fh.get_commit_root()
    flip_low_bit(fh, files, enc // 2, rows // 2)
    os.remove(fh.get_merkle_file_handle())
    with pytest.raises((PF.UnrecoverableError, OSError)):       # the parent's behaviour, kept without locate
        fh.repair(expected_root=root)
    rep = fh.scrub(expected_root=root, locate=True)
    assert rep.bad_columns == [] and not rep.tree_consistent and rep.located_columns == [enc // 2]
    done = fh.repair(expected_root=root, locate=True)
    assert done.repaired_from.startswith("located") and done.located_columns == [enc // 2]
    T.check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_repair_with_a_truncated_tree_and_a_sound_raw_file(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    flip_low_bit(fh, files, 1, 0)
    with open(fh.get_merkle_file_handle(), "r+b") as f:
        f.truncate(len(files["portree"]) - 32)
    with pytest.raises(PF.UnrecoverableError):
        fh.repair()
    done = fh.repair(locate=True)
    assert done.repaired_from.startswith("located") and done.located_columns == [1]
    T.check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_repair_with_too_many_overwritten_leaves(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    root = fh.get_commit_root()
    T.poke(fh.get_merkle_file_handle(), 0, b"\x5a" * (32 * (enc - pre + 1)))   # a run in the leaf area
    flip_low_bit(fh, files, enc - 1, rows - 1)
    damage_raw(fh, files)
    before = T.snapshot(fh)
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(expected_root=root)
    assert T.snapshot(fh) == before
    done = fh.repair(expected_root=root, locate=True)
    assert done.repaired_from.startswith("located") and done.located_columns == [enc - 1]
    assert set(done.repaired_from.split("+")) == {"located", "columns", "tree", "raw"}
    T.check_repaired(fh, files)


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_no_anchor_nothing_written(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    """tree missing, no root, raw file damaged: the code's self-consistency alone is no anchor"""
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    flip_low_bit(fh, files, 0, 0)
    os.remove(fh.get_merkle_file_handle())
    damage_raw(fh, files)
    before = snapshot3(fh)
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(locate=True)
    assert snapshot3(fh) == before and not os.path.exists(fh.get_merkle_file_handle())


def snapshot3(fh):
    d = os.path.dirname(fh.get_encoded_file_handle())
    return {e: T._read(os.path.join(d, f"{T.ULID}.{e}")) for e in T.EXTS if os.path.exists(os.path.join(d, f"{T.ULID}.{e}"))}


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_a_row_beyond_its_radius_is_refused(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    root = fh.get_commit_root()
    t = (enc - pre) // 2 + 1
    row = rows - 1
    for c in T.pick(enc, t, rows):
        T.poke(fh.get_encoded_file_handle(), (c * fh.row_capacity + row) * WB, canonical_junk(oracle, 1, 50 + c))
    os.remove(fh.get_merkle_file_handle())
    damage_raw(fh, files)
    before = snapshot3(fh)
    rep = fh.scrub(expected_root=root, locate=True)
    assert rep.unlocatable_rows == 1 and rep.located_columns == []
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(expected_root=root, locate=True)
    assert snapshot3(fh) == before and not os.path.exists(fh.get_merkle_file_handle())


@pytest.mark.parametrize("pre,enc,rows", CASES)
def test_wrong_expected_root_is_refused(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows):
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows)
    wrong = bytes(b ^ 0xA5 for b in fh.get_commit_root())
    flip_low_bit(fh, files, 0, 0)
    os.remove(fh.get_merkle_file_handle())
    before = snapshot3(fh)
    with pytest.raises(PF.UnrecoverableError):
        fh.repair(expected_root=wrong, locate=True)
    assert snapshot3(fh) == before and not os.path.exists(fh.get_merkle_file_handle())


def test_located_repair_rebuilds_the_chunk_cache(PF, oracle, tmp_path_factory, tmp_path):
    pre, enc, rows = 16, 32, 300
    fh, files = T.store(PF, oracle, tmp_path_factory, tmp_path, pre, enc, rows, chunk_cache=True)
    root = fh.get_commit_root()
    junk_columns(oracle, fh, [4, 9], 8)
    os.remove(fh.get_merkle_file_handle())
    assert fh.repair(expected_root=root, locate=True).repaired_from == "located+columns+tree"
    T.check_repaired(fh, files)
    data = T._read(fh.chunk_cv_file_handle)
    n = PF.check_chunk_cv_sidecar(data[:64], len(data), enc, rows, root)
    assert n == fh.chunk_cache.n_chunks
    assert data[64:64 + n * enc * 32] == fh.chunk_cache.copy_cvs().tobytes()
