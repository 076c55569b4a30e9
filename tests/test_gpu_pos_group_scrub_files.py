"""GPU: a store of small files scrubbed in grouped passes (pos_files.scrub_files over
lcpc_pos_scrub_files_grouped): the reports equal a loop of FileHandler.scrub field by field,
clean and after every kind of damage, and a clean store needs no per-file locate."""
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
# (size, pre, enc): None = the default dims of the size; one empty file
FILES = [(1000, None, None), (65536, None, None), (0, 8, 16), (30_001, None, None), (7 * 64 * 9 - 11, 64, 128),
         (5000, 24, 32), (777, 1, 2), (20_000, 100, 256), (9000, 8, 16), (3000, 15, 16), (56, 8, 16), (12_345, 24, 32)] * 2
DAMAGED = 7      # (20_000, 100, 256): the file every damage goes to; its neighbours stay clean


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def store(gpu, pos, PF, tmp_path_factory):
    """(handlers, roots, baseline): 24 stored files, the roots their owner holds (one of them wrong), and
    the loop of FileHandler.scrub over the clean store for every (locate, with roots)"""
    d = tmp_path_factory.mktemp("scrub_store")
    up, directory = str(d / "up"), str(d / "store")
    os.makedirs(up)
    os.makedirs(directory)
    rng = np.random.default_rng(31)
    specs = []
    for i, (n, pre, enc) in enumerate(FILES):
        if pre is None:
            pre, enc = pos.get_aspect_ratio_default_from_file_len(n)[:2]
        src = os.path.join(up, f"upload_{i}.bin")
        with open(src, "wb") as f:
            f.write(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        specs.append((f"01HSCRUB{i:018d}", src, pre, enc))
    handlers = PF.FileHandler.create_from_unencoded_files(specs, directory)
    roots = [h.get_commit_root() for h in handlers]
    roots[4] = bytes(32)                                   # an owner who holds another root
    baseline = {(locate, with_roots): [h.scrub(expected_root=r if with_roots else None, locate=locate)
                                       for h, r in zip(handlers, roots)]
                for locate in (False, True) for with_roots in (False, True)}
    return handlers, roots, baseline


def same(a, b):
    return dataclasses.asdict(a) == dataclasses.asdict(b)


def check_against_loop(PF, store, touched):
    """scrub_files over the whole store for every (locate, with roots) against the loop: the baseline for
    the untouched files, a fresh FileHandler.scrub for the touched ones"""
    handlers, roots, baseline = store
    for (locate, with_roots), base in baseline.items():
        er = roots if with_roots else None
        got = PF.scrub_files(handlers, er, locate=locate)
        assert len(got) == len(handlers)
        for i, (h, g) in enumerate(zip(handlers, got)):
            want = h.scrub(expected_root=roots[i] if with_roots else None, locate=locate) if i in touched else base[i]
            assert same(g, want), (i, locate, with_roots, g, want)
    return got


class patched:
    """a file changed on disk for the length of a with block"""

    def __init__(self, path, change):
        self.path, self.change = path, change

    def __enter__(self):
        with open(self.path, "rb") as f:
            self.saved = f.read()
        new = self.change(bytearray(self.saved))
        if new is None:
            os.remove(self.path)
        else:
            with open(self.path, "wb") as f:
                f.write(bytes(new))

    def __exit__(self, *exc):
        with open(self.path, "wb") as f:
            f.write(self.saved)


def test_clean_store(PF, store):
    handlers, roots, baseline = store
    got = check_against_loop(PF, store, touched=())
    assert all(r.clean for i, r in enumerate(baseline[(True, False)])) and len(got) == len(FILES)
    assert [i for i, r in enumerate(baseline[(True, True)]) if not r.clean] == [4]
    assert all(r.located_columns == [] and r.unlocatable_rows == 0 for r in got)
    assert PF.scrub_files([]) == []
    with pytest.raises(ValueError):
        PF.scrub_files(handlers, roots[:3])


def test_damaged_porenc_byte(PF, store):
    h = store[0][DAMAGED]
    at = (5 * h.row_capacity + 2) * 8          # column 5, row 2, the low byte: the value stays canonical

    def flip(b):
        b[at] ^= 0x01
        return b
    with patched(h.encoded_file_handle, flip):
        got = check_against_loop(PF, store, {DAMAGED})
    assert got[DAMAGED].bad_columns == [5] and got[DAMAGED].located_columns == [5]
    assert got[DAMAGED].noncanonical_columns == [] and got[DAMAGED].unlocatable_rows == 0


def test_noncanonical_column(PF, store):
    h = store[0][DAMAGED]
    lo = 9 * h.row_capacity * 8

    def ff(b):
        b[lo:lo + 8 * h.rows_written] = b"\xff" * (8 * h.rows_written)
        return b
    with patched(h.encoded_file_handle, ff):
        got = check_against_loop(PF, store, {DAMAGED})
    assert got[DAMAGED].bad_columns == [9] and got[DAMAGED].noncanonical_columns == [9]
    assert got[DAMAGED].located_columns == [9]


def test_truncated_tree(PF, store):
    handlers, roots, baseline = store
    h = handlers[DAMAGED]
    with patched(h.merkle_tree_file_handle, lambda b: b[:-32]):
        for with_roots in (False, True):
            er = roots if with_roots else None
            got = PF.scrub_files(handlers, er, locate=True)
            for i, (x, g) in enumerate(zip(handlers, got)):
                want = x.scrub(expected_root=roots[i] if with_roots else None, locate=True) if i == DAMAGED \
                    else baseline[(True, with_roots)][i]
                assert same(g, want), (i, with_roots, g, want)
            assert got[DAMAGED].tree_consistent is False and got[DAMAGED].bad_columns == []
            assert got[DAMAGED].located_columns == [] and got[DAMAGED].raw_ok is False
            with pytest.raises(PF.UnrecoverableError):
                h.scrub(expected_root=er and roots[DAMAGED])
            with pytest.raises(PF.UnrecoverableError):
                PF.scrub_files(handlers, er)
    # a tree file that is not there at all
    with patched(h.merkle_tree_file_handle, lambda b: None):
        got = PF.scrub_files(handlers[DAMAGED - 1:DAMAGED + 2], None, locate=True)
        assert same(got[1], h.scrub(locate=True)) and same(got[0], baseline[(True, False)][DAMAGED - 1])
        with pytest.raises(OSError):
            h.scrub()
        with pytest.raises(OSError):
            PF.scrub_files(handlers)


def test_deleted_raw_file(PF, store):
    h = store[0][DAMAGED]
    with patched(h.unencoded_file_handle, lambda b: None):
        got = check_against_loop(PF, store, {DAMAGED})
    assert got[DAMAGED].raw_ok is False and got[DAMAGED].bad_columns == [] and got[DAMAGED].tree_consistent


def test_changed_raw_byte(PF, store):
    h = store[0][DAMAGED]

    def change(b):
        b[1234] ^= 0x40
        return b
    with patched(h.unencoded_file_handle, change):
        got = check_against_loop(PF, store, {DAMAGED})
    assert got[DAMAGED].raw_ok is False and got[DAMAGED].bad_columns == []
    # a raw file of another length does not join the grouped encode
    with patched(h.unencoded_file_handle, lambda b: b[:-1]):
        got = check_against_loop(PF, store, {DAMAGED})
    assert got[DAMAGED].raw_ok is False


def test_clean_store_needs_no_per_file_device_call(gpu, PF, store):
    handlers, roots, baseline = store
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = PF.scrub_files(handlers, roots, locate=True)
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert all(same(g, w) for g, w in zip(got, baseline[(True, True)]))
    assert stats["pos_group_scrub"][1] >= 1 and stats["pos_group_ingest"][1] >= 1
    # nothing of the per-file scrub, locate or encode ran: only the two grouped legs' regions are there
    assert all(name.startswith(("pos_group_scrub", "pos_group_ingest")) for name in stats), sorted(stats)
    # a file with a finding does reach the per-file locator
    h = handlers[DAMAGED]

    def flip(b):
        b[(3 * h.row_capacity + 1) * 8] ^= 0x01
        return b
    with patched(h.encoded_file_handle, flip):
        gpu.prof_enable(True)
        try:
            gpu.prof_reset()
            got = PF.scrub_files(handlers, roots, locate=True)
            stats = gpu.prof_stats()
        finally:
            gpu.prof_enable(False)
            gpu.prof_reset()
    assert got[DAMAGED].located_columns == [3] and any(name.startswith("rs_locate") for name in stats), sorted(stats)
