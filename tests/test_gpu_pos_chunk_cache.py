"""GPU: incremental Merkle updates of stored proof-of-storage files -- the column chunk-CV cache
(pos_files.ColumnChunkCache over lcpc_pos_chunk_cache_*, FileHandler(chunk_cache=True)).

* the non-clobbering fold (lcpc_leaves_fold_cvs) equals lcpc_leaves_from_cvs and leaves its input;
* the cached chaining values equal pure-Python BLAKE3 chunk CVs (pyref) and the writer's own;
* after every edit and append the `.porenc` and the tree equal the oracle's fresh encode of the
  edited contents, the tree equals a chunk_cache=False handler's, and the rehashed chunk range is
  the one lcpc_pos_update_chunk_range states;
* the `.porcv` sidecar is loaded when it belongs to the file and rebuilt when it does not;
* a non-canonical element fails the update as it fails lcpc_pos_porenc_tree, the cache unchanged;
* the empty ColumnDigestAccumulator gives BLAKE3(32 zero bytes) per column.
"""
import os

import numpy as np
import pytest

import pyref

pytestmark = pytest.mark.gpu
WB = 8
DIMS = [(2, 4), (16, 32)]     # a row is 14 or 112 data bytes


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


@pytest.fixture(scope="module")
def N(gpu):
    from lcpc_proof_of_storage_amd import _native
    _native.load()
    return _native


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _check_against_oracle(fh, oracle, contents):
    """the .porenc columns (first rows_written elements) and the tree equal a fresh encode"""
    pre, enc, rows = fh.get_dimensions()
    img, otree, orows, ocap = oracle.pos_encode_file(contents, pre, enc)
    assert orows == rows
    got = np.frombuffer(_read(fh.get_encoded_file_handle()), np.uint8).reshape(enc, -1)[:, :rows * WB]
    want = np.frombuffer(img, np.uint8).reshape(enc, -1)[:, :rows * WB]
    assert np.array_equal(got, want)
    assert fh.get_merkle_tree().to_bytes() == otree
    assert _read(fh.get_merkle_file_handle()) == otree


def _create(PF, tmp_path, name, contents, pre, enc, chunk_cache, ulid="01CHUNKCACHETEST0000000000"):
    src = tmp_path / f"{name}.bin"
    src.write_bytes(contents)
    return PF.FileHandler.create_from_unencoded_file(ulid, str(src), pre, enc, directory=str(tmp_path / name),
                                                     chunk_cache=chunk_cache)


def _sidecar_matches_cache(PF, fh):
    data = _read(fh.chunk_cv_file_handle)
    pre, enc, rows = fh.get_dimensions()
    n = PF.check_chunk_cv_sidecar(data[:64], len(data), enc, rows, fh.get_merkle_tree().root())
    assert n == fh.chunk_cache.n_chunks and fh.chunk_cache.rows == rows and fh.chunk_cache.enc == enc
    assert data[64:64 + n * enc * 32] == fh.chunk_cache.copy_cvs().tobytes()


# ---------------------------------------------------------------- the fold
@pytest.mark.parametrize("n_cols", [4, 32, 4096])
def test_fold_equals_leaves_from_cvs_and_keeps_its_input(N, n_cols):
    """every chunk count 1..9, 16, 17, 74 (the 1 GiB file's), and 257 / 300 for the deeper stack"""
    lib = N.load()
    rng = np.random.default_rng(n_cols)
    for n_chunks in list(range(1, 10)) + [16, 17, 74] + ([257, 300] if n_cols <= 32 else []):
        cvs = rng.integers(0, 256, (n_chunks, n_cols, 32), dtype=np.uint8)
        keep = cvs.copy()
        want = np.zeros((n_cols, 32), np.uint8)
        assert lib.lcpc_leaves_from_cvs(cvs.ctypes.data_as(N.u8p), n_chunks, n_cols, want.ctypes.data_as(N.u8p)) == 0
        got = np.zeros((n_cols, 32), np.uint8)
        after = np.zeros_like(cvs)
        assert lib.lcpc_leaves_fold_cvs(cvs.ctypes.data_as(N.u8p), n_chunks, n_cols, got.ctypes.data_as(N.u8p),
                                        after.ctypes.data_as(N.u8p)) == 0
        assert np.array_equal(got, want), n_chunks
        assert np.array_equal(after, keep) and np.array_equal(cvs, keep), n_chunks


def test_fold_small_counts_match_pyref(N):
    """the fold against BLAKE3's own merge rule on whole messages (pure Python), enc = 4"""
    lib = N.load()
    rng = np.random.default_rng(11)
    for n_chunks in [1, 2, 3, 5, 8]:
        msgs = [rng.integers(0, 256, 1024 * n_chunks - 37, dtype=np.uint8).tobytes() for _ in range(4)]
        cvs = np.zeros((n_chunks, 4, 32), np.uint8)
        for c, m in enumerate(msgs):
            for i in range(n_chunks):
                cv = pyref._chunk_cv(m[1024 * i:1024 * (i + 1)], i, n_chunks == 1)
                cvs[i, c] = np.frombuffer(b"".join(x.to_bytes(4, "little") for x in cv), np.uint8)
        got = np.zeros((4, 32), np.uint8)
        assert lib.lcpc_leaves_fold_cvs(cvs.ctypes.data_as(N.u8p), n_chunks, 4, got.ctypes.data_as(N.u8p), None) == 0
        assert [g.tobytes() for g in got] == [pyref.blake3(m) for m in msgs]


# ---------------------------------------------------------------- chaining-value parity
def _pyref_cvs(image, enc, rows, cap):
    n = max(1, -(-(32 + 8 * rows) // 1024))
    out = np.zeros((n, enc, 32), np.uint8)
    for c in range(enc):
        msg = bytes(32) + bytes(image[c * cap * WB:(c * cap + rows) * WB])
        for i in range(n):
            cv = pyref._chunk_cv(msg[1024 * i:1024 * (i + 1)], i, n == 1)
            out[i, c] = np.frombuffer(b"".join(x.to_bytes(4, "little") for x in cv), np.uint8)
    return out


@pytest.mark.parametrize("pre,enc", DIMS)
@pytest.mark.parametrize("rows", [0, 1, 124, 125, 252, 300, 600])
def test_cvs_match_pyref_and_writer(PF, tmp_path, pre, enc, rows):
    contents = _bytes(max(rows * pre * 7 - 3, 0), rows + enc)
    with open(tmp_path / "img.porenc", "w+b") as f:
        w = PF.EncodedFileWriter(pre, enc, len(contents), f)
        if contents:
            w.push_bytes(contents)
        meta, tree = w.finalize_to_merkle_tree(keep_chunk_cvs=True)
    assert meta.rows_written == rows
    image = np.fromfile(tmp_path / "img.porenc", np.uint8)
    cache = PF.ColumnChunkCache.from_porenc(image, enc, rows, meta.row_capacity)
    assert (cache.enc, cache.rows, cache.n_chunks) == (enc, rows, PF.leaf_n_chunks(rows))
    got = cache.copy_cvs()
    assert np.array_equal(got, w.chunk_cvs)
    if enc == 4:  # (pure-Python BLAKE3)
        assert np.array_equal(got, _pyref_cvs(image, enc, rows, meta.row_capacity))
    assert cache.tree() == tree
    assert np.array_equal(cache.digests(), tree.digests[:enc])
    if cache.n_chunks > 1:
        assert np.array_equal(cache.copy_cvs(1, 2), got[1:2])
    again = PF.ColumnChunkCache.from_cvs(got, enc, rows)
    assert again.tree() == tree and np.array_equal(again.copy_cvs(), got)
    with pytest.raises(ValueError):
        PF.ColumnChunkCache.from_cvs(got[:, :-1], enc, rows)


# ---------------------------------------------------------------- edits
def _edit_rows(rows):
    """(first row, end row) of each edit: row 0, the rows straddling chunks 0 | 1 and 1 | 2, a
    mid-chunk row, the last row (in the short last chunk), and rows spanning three chunks"""
    return [(0, 1), (123, 125), (251, 253), (190, 191), (rows - 1, rows), (120, 260)]


@pytest.mark.parametrize("pre,enc", DIMS)
@pytest.mark.parametrize("rows", [300, 900])
def test_edits(PF, oracle, tmp_path, pre, enc, rows):
    rb = pre * 7
    contents = bytearray(_bytes(rows * rb - 3, rows + pre))   # the last row is short
    fh = _create(PF, tmp_path, "cached", bytes(contents), pre, enc, True)
    plain = _create(PF, tmp_path, "plain", bytes(contents), pre, enc, False)
    assert fh.get_dimensions() == (pre, enc, rows) and fh.chunk_cache.n_chunks == PF.leaf_n_chunks(rows)
    assert not os.path.exists(plain.chunk_cv_file_handle) and plain.chunk_cache is None
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(
        f"01CHUNKCACHETEST0000000000.{e}" for e in ("porraw", "porenc", "portree", "meta"))
    _sidecar_matches_cache(PF, fh)
    rng = np.random.default_rng(rows)
    for row_lo, row_hi in _edit_rows(rows):
        start, end = row_lo * rb, min(row_hi * rb, len(contents))
        new = rng.integers(0, 256, end - start, dtype=np.uint8).tobytes()
        old, tree = fh.edit_bytes(start, new)
        assert old == bytes(contents[start:end])
        contents[start:end] = new
        _, plain_tree = plain.edit_bytes(start, new)
        _check_against_oracle(fh, oracle, bytes(contents))
        assert tree == plain_tree and _read(fh.get_merkle_file_handle()) == _read(plain.get_merkle_file_handle())
        assert _read(fh.get_encoded_file_handle()) == _read(plain.get_encoded_file_handle())
        assert _read(fh.metadata_file_handle) == _read(plain.metadata_file_handle)
        assert fh.last_chunk_range == PF.ColumnChunkCache.update_chunk_range(rows, rows, row_lo, row_hi)
        _sidecar_matches_cache(PF, fh)
    fh.verify_all_files_agree()
    plain.delete_all_files()
    fh.delete_all_files()
    assert not os.path.exists(tmp_path / "cached")


# ---------------------------------------------------------------- appends
@pytest.mark.parametrize("pre,enc", DIMS)
def test_appends_from_the_empty_file(PF, oracle, tmp_path, pre, enc):
    rb = pre * 7
    fh = _create(PF, tmp_path, "cached", b"", pre, enc, True)
    assert fh.get_dimensions()[2] == 0 and fh.chunk_cache.n_chunks == 1
    assert [d.tobytes() for d in fh.chunk_cache.digests()] == [pyref.blake3(bytes(32))] * enc
    _sidecar_matches_cache(PF, fh)
    contents = bytearray()
    # rows after each step: inside chunk 0; exactly chunk 0 full (124), then one more (1 -> 2 chunks:
    # ROOT leaves chunk 0); exactly two chunks full (252), then one more; across two chunk
    # boundaries (380 and 508) in one call; past the row capacity (the image is re-laid out)
    relaid = False
    for target_rows in [1, 100, 124, 125, 252, 253, 513, 1100]:
        old_rows, old_cap = fh.rows_written, fh.row_capacity
        n = target_rows * rb - len(contents) - (5 if target_rows in (1, 513) else 0)   # (short last rows too)
        new = _bytes(n, target_rows)
        start_row = len(contents) // rb
        tree = fh.append_bytes(new)
        contents += new
        assert fh.rows_written == target_rows and _read(fh.get_raw_file_handle()) == bytes(contents)
        _check_against_oracle(fh, oracle, bytes(contents))
        assert tree == fh.recalculate_tree_only()
        assert fh.last_chunk_range == PF.ColumnChunkCache.update_chunk_range(old_rows, target_rows, start_row,
                                                                             target_rows)
        assert fh.last_chunk_range[1] == PF.leaf_n_chunks(target_rows)
        _sidecar_matches_cache(PF, fh)
        relaid |= old_rows > 0 and fh.row_capacity != old_cap
    assert relaid
    fh.verify_all_files_agree()
    # a few bytes more, and an empty append
    for new in [b"xyz", b""]:
        fh.append_bytes(new)
        contents += new
        _check_against_oracle(fh, oracle, bytes(contents))
    again = PF.FileHandler.new_attach_to_existing_ulid(str(tmp_path / "cached"), fh.file_ulid, chunk_cache=True)
    assert again.get_encoded_metadata() == fh.get_encoded_metadata()
    assert np.array_equal(again.chunk_cache.copy_cvs(), fh.chunk_cache.copy_cvs())
    fh.delete_all_files()
    assert not os.path.exists(tmp_path / "cached")


# ---------------------------------------------------------------- persistence
def test_sidecar_is_loaded_or_rebuilt(PF, oracle, tmp_path, monkeypatch):
    pre, enc, rows = 2, 4, 300
    rb = pre * 7
    contents = bytearray(_bytes(rows * rb, 21))
    fh = _create(PF, tmp_path, "cached", bytes(contents), pre, enc, True)
    new = _bytes(3 * rb, 22)
    fh.edit_bytes(100 * rb, new)
    contents[100 * rb:103 * rb] = new
    want_cvs, sidecar = fh.chunk_cache.copy_cvs(), _read(fh.chunk_cv_file_handle)
    d, ulid = str(tmp_path / "cached"), fh.file_ulid

    # present and right: loaded, not rebuilt
    with monkeypatch.context() as mp:
        def no_rebuild(self):
            raise AssertionError("the sidecar should have been loaded")
        mp.setattr(PF.FileHandler, "_rebuild_chunk_cache", no_rebuild)
        again = PF.FileHandler.new_attach_to_existing_ulid(d, ulid, chunk_cache=True)
        assert np.array_equal(again.chunk_cache.copy_cvs(), want_cvs)

    def deleted(p):
        os.remove(p)

    def truncated(p):
        with open(p, "r+b") as f:
            f.truncate(len(sidecar) - 40)

    def bad_magic(p):
        with open(p, "r+b") as f:
            f.write(b"X")

    def bad_root(p):
        with open(p, "r+b") as f:
            f.seek(40)
            f.write(bytes([sidecar[40] ^ 1]))

    def bad_rows(p):
        with open(p, "r+b") as f:
            f.seek(16)
            f.write((rows + 1).to_bytes(8, "little"))

    def bad_body(p):
        with open(p, "r+b") as f:
            f.seek(64 + 32 * enc + 7)
            f.write(bytes([sidecar[64 + 32 * enc + 7] ^ 0x80]))

    rng = np.random.default_rng(23)
    for k, damage in enumerate([deleted, truncated, bad_magic, bad_root, bad_rows, bad_body]):
        damage(fh.chunk_cv_file_handle)
        rebuilt = []
        with monkeypatch.context() as mp:
            real = PF.FileHandler._rebuild_chunk_cache
            mp.setattr(PF.FileHandler, "_rebuild_chunk_cache", lambda self: rebuilt.append(1) or real(self))
            again = PF.FileHandler.new_attach_to_existing_ulid(d, ulid, chunk_cache=True)
        assert rebuilt == [1], damage.__name__
        assert np.array_equal(again.chunk_cache.copy_cvs(), want_cvs), damage.__name__
        assert _read(fh.chunk_cv_file_handle) == sidecar, damage.__name__
        # edits through the re-attached handler stay correct
        row = int(rng.integers(0, rows))
        new = _bytes(rb, 30 + k)
        again.edit_bytes(row * rb, new)
        contents[row * rb:(row + 1) * rb] = new
        _check_against_oracle(again, oracle, bytes(contents))
        _sidecar_matches_cache(PF, again)
        want_cvs, sidecar = again.chunk_cache.copy_cvs(), _read(fh.chunk_cv_file_handle)
    again.verify_all_files_agree()
    # a handler without the cache edits the file: the sidecar goes stale and the next attach rebuilds it
    plain = PF.FileHandler.new_attach_to_existing_ulid(d, ulid)
    new = _bytes(rb, 40)
    plain.edit_bytes(7 * rb, new)
    contents[7 * rb:8 * rb] = new
    assert _read(fh.chunk_cv_file_handle) == sidecar
    again = PF.FileHandler.new_attach_to_existing_ulid(d, ulid, chunk_cache=True)
    _check_against_oracle(again, oracle, bytes(contents))
    again.verify_all_files_agree()
    # a handler without the cache still removes the sidecar an earlier one left
    assert os.path.isfile(again.chunk_cv_file_handle)
    PF.FileHandler.new_attach_to_existing_ulid(d, ulid).delete_all_files()
    assert not os.path.exists(d)


def test_reshape_and_reencode_keep_the_cache(PF, oracle, tmp_path):
    contents = bytearray(_bytes(10000, 31))
    fh = _create(PF, tmp_path, "cached", bytes(contents), 16, 32, True)
    fh.reshape(8, 16)
    assert fh.chunk_cache.enc == 16 and fh.chunk_cache.rows == fh.rows_written
    fh.verify_all_files_agree()
    _sidecar_matches_cache(PF, fh)
    new = _bytes(200, 32)
    fh.edit_bytes(5000, new)
    contents[5000:5200] = new
    _check_against_oracle(fh, oracle, bytes(contents))
    fh.reencode_unencoded_file()
    fh.verify_all_files_agree()
    _sidecar_matches_cache(PF, fh)
    fh.append_bytes(b"tail" * 100)
    contents += b"tail" * 100
    _check_against_oracle(fh, oracle, bytes(contents))
    fh.delete_all_files()


def test_non_canonical_element_fails_the_update_and_keeps_the_cache(PF, tmp_path):
    pre, enc, rows = 2, 4, 300
    p = pyref.FIELD_DECL[0][0]
    contents = _bytes(rows * pre * 7, 41)
    with open(tmp_path / "img.porenc", "w+b") as f:
        w = PF.EncodedFileWriter(pre, enc, len(contents), f)
        w.push_bytes(contents)
        meta, tree = w.finalize_to_merkle_tree()
    cap = meta.row_capacity
    image = np.fromfile(tmp_path / "img.porenc", np.uint8)
    cache = PF.ColumnChunkCache.from_porenc(image, enc, rows, cap)
    before = cache.copy_cvs()
    bad = image.copy()
    bad.view("<u8").reshape(enc, cap)[1, 130] = p          # row 130: chunk 1
    with open(tmp_path / "bad.porenc", "wb") as f:
        f.write(bad.tobytes())
    with open(tmp_path / "bad.porenc", "rb") as f, pytest.raises(Exception) as full_pass:
        PF.EncodedFileReader.new_ligero(f, pre, enc, rows, cap).process_file_to_merkle_tree()
    with pytest.raises(full_pass.type) as e:
        cache.update(bad, cap, 130, 131, rows)
    assert e.value.code == full_pass.value.code and "canonical" in str(e.value)
    assert np.array_equal(cache.copy_cvs(), before) and cache.rows == rows and cache.tree() == tree
    with pytest.raises(full_pass.type):            # growth over the bad chunk fails too, nothing grown
        cache.update(bad, cap, 130, 301, 301)
    assert np.array_equal(cache.copy_cvs(), before) and (cache.rows, cache.n_chunks) == (rows, 3)
    with pytest.raises(full_pass.type):
        PF.ColumnChunkCache.from_porenc(bad, enc, rows, cap)
    # the same through the file (pread) form, and a file that ends before a slice
    with open(tmp_path / "bad.porenc", "rb") as f:
        with pytest.raises(full_pass.type) as e:
            cache.update_file(f, cap, 130, 131, rows)
        assert "canonical" in str(e.value)
        assert cache.update_file(f, cap, 0, 1, rows) == (0, 1)
    with open(tmp_path / "short.porenc", "wb") as f:
        f.write(image[:3 * cap * WB + 100 * WB].tobytes())       # column 3 ends at row 100
    with open(tmp_path / "short.porenc", "rb") as f, pytest.raises(full_pass.type):
        cache.update_file(f, cap, 130, 131, rows)
    assert np.array_equal(cache.copy_cvs(), before) and cache.tree() == tree
    # p - 1 is canonical; and chunks the update does not touch are not read
    ok = image.copy()
    ok.view("<u8").reshape(enc, cap)[1, 130] = p - 1
    assert cache.update(ok, cap, 130, 131, rows) == (1, 2)
    assert cache.update(bad, cap, 0, 1, rows) == (0, 1)
    with pytest.raises(full_pass.type):            # a shrinking row count
        cache.update(image, cap, 0, 1, rows - 1)


# ---------------------------------------------------------------- the empty accumulator
@pytest.mark.parametrize("field", [0, 1])
def test_empty_column_digest_accumulator(PF, field):
    want = pyref.blake3(bytes(32))
    acc = PF.ColumnDigestAccumulator(8, PF.ColumnsToCareAbout.All, field)
    assert acc.get_column_digests() == [want] * 8
    acc = PF.ColumnDigestAccumulator(8, PF.ColumnsToCareAbout.All, field)
    acc.update(np.zeros((0, 8 * (field + 1)), np.uint64))
    tree = acc.finalize_to_merkle_tree()
    assert [tree[i] for i in range(8)] == [want] * 8
    assert tree[8] == pyref.blake3(want + want)
