"""GPU: a store of small files repaired in grouped passes (pos_files.repair_files over
lcpc_pos_scrub_files_grouped and lcpc_pos_repair_files_grouped).  Two copies of one store are
damaged identically; one is repaired by repair_files, the other by the loop of FileHandler.repair: the
reports are equal field by field, the exceptions of one type at the same indices, and every file on disk
is byte-identical between the two stores."""
import dataclasses
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
# (size, pre, enc, chunk_cache): 24 files at dims (16, 32) and (128, 256)
FILES = [(n, pre, enc, cc) for cc in (False, True, False) for n, pre, enc in
         ((5000, 16, 32), (20_000, 128, 256), (777, 16, 32), (65_536, 128, 256), (112 * 9, 16, 32), (30_001, 128, 256),
          (12_345, 16, 32), (9000, 128, 256))]
EXT = ("porraw", "porenc", "portree", "meta", "porcv")


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def build_store(PF, d):
    """(handlers of store a, handlers of its copy b, roots)"""
    up, a, b = str(d / "up"), str(d / "a"), str(d / "b")
    os.makedirs(up)
    os.makedirs(a)
    rng = np.random.default_rng(47)
    ha = [None] * len(FILES)
    for cc in (False, True):
        specs, idx = [], []
        for i, (n, pre, enc, c) in enumerate(FILES):
            if c != cc:
                continue
            src = os.path.join(up, f"upload_{i}.bin")
            with open(src, "wb") as f:
                f.write(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
            specs.append((f"01HREPAIR{i:017d}", src, pre, enc))
            idx.append(i)
        for i, h in zip(idx, PF.FileHandler.create_from_unencoded_files(specs, a, chunk_cache=cc)):
            ha[i] = h
    shutil.copytree(a, b)
    hb = [PF.FileHandler.new_attach_to_existing_ulid(b, h.file_ulid, chunk_cache=FILES[i][3]) for i, h in enumerate(ha)]
    return ha, hb, [h.get_commit_root() for h in ha]


def change(path, fn):
    with open(path, "rb") as f:
        data = bytearray(f.read())
    new = fn(data)
    if new is None:
        os.remove(path)
    else:
        with open(path, "wb") as f:
            f.write(bytes(new))


def flip_elems(h, cols, row=0, bit=0x01):
    """the low byte of element (col, row) of every listed column: the values stay canonical"""
    def fn(b):
        for c in cols:
            b[(c * h.row_capacity + row) * 8] ^= bit
        return b
    return fn


def ff_column(h, col):
    def fn(b):
        lo = col * h.row_capacity * 8
        b[lo:lo + 8 * h.rows_written] = b"\xff" * (8 * h.rows_written)
        return b
    return fn


def flip_byte(at):
    def fn(b):
        b[at] ^= 0x10
        return b
    return fn


def damages(h):
    """index of FILES -> list of (file of the handler, change); clean files in between (8 .. 15 keep a
    chunk cache)"""
    w, pre = h.encoded_size, h.pre_encoded_size
    enc, tree, raw = "encoded_file_handle", "merkle_tree_file_handle", "unencoded_file_handle"
    return {
        0: [(enc, flip_elems(h, [5], row=2))],                                   # a flipped .porenc byte
        1: [(enc, ff_column(h, 9))],                                             # a 0xFF column
        2: [(enc, flip_elems(h, range(3, 3 + 7), row=1))],                       # a run of columns
        4: [(tree, flip_byte(32 * 6 + 3))],                                      # a stored leaf
        5: [(tree, flip_byte(32 * (w + 7) + 31))],                               # a stored parent
        6: [(tree, flip_byte(32 * (2 * w - 2)))],                                # the stored root
        8: [(enc, flip_elems(h, range(w - pre + 1)))],                           # too many columns, sound raw file
        9: [(enc, flip_elems(h, range(w - pre + 1))), (raw, flip_byte(100))],    # ... and a damaged raw file
        10: [(tree, lambda b: b[:-32])],                                         # a truncated .portree
        12: [(tree, lambda b: None)],                                            # a missing .portree
        13: [(raw, lambda b: b[:-1])],                                           # a shortened raw file
        14: [(enc, flip_elems(h, [0, w - 1], row=0)), (tree, flip_byte(32 * 2))],  # columns and a leaf
        16: [(enc, flip_elems(h, [11]))],
        17: [(enc, ff_column(h, 200)), (enc, flip_elems(h, [3, 4, 5]))],
        19: [(raw, flip_byte(7))],
        21: [(enc, flip_elems(h, range(w - pre)))],                              # exactly enc - pre columns
        22: [(enc, flip_elems(h, [31], row=3)), (raw, lambda b: None)],
    }


def files_of(h):
    d = os.path.dirname(h.encoded_file_handle)
    return [os.path.join(d, f"{h.file_ulid}.{e}") for e in EXT]


def read_or_none(p):
    try:
        with open(p, "rb") as f:
            return f.read()
    except OSError:
        return None


def loop_repair(PF, handlers, roots, locate):
    out = []
    for h, r in zip(handlers, roots):
        try:
            out.append(h.repair(expected_root=r, locate=locate))
        except (PF.UnrecoverableError, OSError) as e:
            out.append(e)
    return out


@pytest.mark.parametrize("locate,with_roots", [(False, True), (True, True), (False, False), (True, False)])
def test_repair_files_equals_the_loop(PF, tmp_path, locate, with_roots):
    ha, hb, roots = build_store(PF, tmp_path)
    er = roots if with_roots else [None] * len(roots)
    for hs in (ha, hb):
        for i, h in enumerate(hs):
            for attr, fn in damages(h).get(i, []):
                change(getattr(h, attr), fn)
    for x, y in zip(ha, hb):                      # damaged identically
        assert [read_or_none(p) for p in files_of(x)] == [read_or_none(p) for p in files_of(y)]
    got = PF.repair_files(ha, er, locate=locate)
    want = loop_repair(PF, hb, er, locate)
    assert len(got) == len(want) == len(FILES)
    mended = []
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, Exception):
            assert type(g) is type(w), (i, g, w)
        else:
            assert isinstance(g, PF.ScrubReport) and dataclasses.asdict(g) == dataclasses.asdict(w), (i, g, w)
            mended.append(i)
    for i, (x, y) in enumerate(zip(ha, hb)):
        for p, q in zip(files_of(x), files_of(y)):
            assert read_or_none(p) == read_or_none(q), (i, p)
    # what the test set up did happen: the grouped files were mended from their columns, some files cannot be
    assert got[0].repaired_from == "columns" and got[1].repaired_from == "columns" and got[21].repaired_from == "columns"
    assert got[3].repaired_from is None and got[8].repaired_from == "reencode"
    assert isinstance(got[9], PF.UnrecoverableError)
    # (9 always; 10 and 12 have no tree file; without roots a damaged tree is no anchor: 4, 5, 6 and 14)
    assert len(mended) >= len(FILES) - (1 if locate else 3 if with_roots else 7)
    # the mended files are whole again
    again = PF.scrub_files([ha[i] for i in mended], [er[i] for i in mended])
    for i, r in zip(mended, again):
        assert r.clean, (i, r)
        ha[i].verify_all_files_agree()


def test_groupable_damage_needs_no_per_file_device_call(gpu, PF, tmp_path):
    ha, _, roots = build_store(PF, tmp_path)
    plain = [i for i, f in enumerate(FILES) if not f[3]]
    hs, rs = [ha[i] for i in plain], [roots[i] for i in plain]
    for k, h in enumerate(hs):
        if k % 3 == 0:
            change(h.encoded_file_handle, flip_elems(h, range(k % 5, k % 5 + 1 + k % 4), row=k % 2))
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = PF.repair_files(hs, rs)
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert [r.repaired_from for r in got] == ["columns" if k % 3 == 0 else None for k in range(len(hs))]
    assert stats["pos_group_scrub"][1] >= 1 and stats["pos_group_ingest"][1] >= 1 and stats["pos_group_repair"][1] == 1
    assert all(name.startswith(("pos_group_scrub", "pos_group_ingest", "pos_group_repair")) for name in stats), sorted(stats)
    assert all(r.clean for r in PF.scrub_files(hs, rs))
    assert PF.repair_files([]) == []
    with pytest.raises(ValueError):
        PF.repair_files(hs, rs[:3])
