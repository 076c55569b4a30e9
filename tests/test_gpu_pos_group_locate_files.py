"""GPU: a store of small files repaired with locate=True in grouped passes (pos_files.repair_files over
lcpc_pos_locate_files_grouped).  Two copies of one store are damaged identically; one goes
through scrub_files(locate=True) / repair_files(locate=True), the other through the loops of
FileHandler.scrub / FileHandler.repair: the reports are equal field by field, the exceptions of one type at
the same indices, and every file on disk is byte-identical between the two stores."""
import dataclasses
import os

import pytest

import test_gpu_pos_group_repair_files as T

pytestmark = pytest.mark.gpu
FILES = T.FILES
GROUPED = ("pos_group_scrub", "pos_group_ingest", "pos_group_locate", "pos_group_repair")


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def damages(h):
    """index of FILES -> list of (file of the handler, change); 8 .. 15 keep a chunk cache"""
    w, pre = h.encoded_size, h.pre_encoded_size
    t = (w - pre) // 2
    enc, tree, raw = "encoded_file_handle", "merkle_tree_file_handle", "unencoded_file_handle"
    return {
        0: [(enc, T.flip_elems(h, [5], row=2))],                                      # a flipped .porenc byte
        1: [(enc, T.ff_column(h, 9))],                                                # a 0xFF column
        2: [(enc, T.flip_elems(h, range(3, 3 + 7), row=1))],                          # a run of columns
        4: [(enc, T.flip_elems(h, range(1, 1 + t), row=0))],                          # t = (enc - pre) / 2 columns
        5: [(enc, T.flip_elems(h, range(w - t - 1, w), row=1))],                      # t + 1 columns, sound raw file
        6: [(tree, lambda b: None), (enc, T.flip_elems(h, [0, w - 1], row=0))],       # a missing .portree, damage
        7: [(tree, lambda b: b[:-32]), (enc, T.flip_elems(h, range(2, 2 + t), row=3))],   # a truncated one
        8: [(tree, lambda b: bytes(len(b))), (enc, T.flip_elems(h, [7], row=1))],     # an overwritten one
        9: [(tree, lambda b: None), (enc, T.ff_column(h, 100)), (enc, T.flip_elems(h, [3, 4], row=2))],
        10: [(tree, lambda b: None)],                                                 # missing, the image sound
        12: [(tree, lambda b: None), (enc, T.flip_elems(h, range(t + 1), row=0))],    # missing, not locatable
        13: [(raw, lambda b: b[:-1])],                                                # a shortened raw file
        14: [(tree, lambda b: b[:-32]), (enc, T.flip_elems(h, [1], row=0)), (raw, T.flip_byte(5))],
        16: [(tree, T.flip_byte(32 * 6 + 3)), (enc, T.flip_elems(h, [11]))],          # a leaf and a column
        17: [(enc, T.ff_column(h, 200)), (enc, T.flip_elems(h, [3, 4, 5]))],
        19: [(tree, lambda b: None), (raw, lambda b: None), (enc, T.flip_elems(h, [2], row=1))],
        21: [(enc, T.flip_elems(h, range(w - pre)))],                                 # exactly enc - pre columns
        22: [(tree, lambda b: b"\xff" * len(b)), (enc, T.flip_elems(h, [31], row=3))],
    }


def damaged_store(PF, tmp_path):
    ha, hb, roots = T.build_store(PF, tmp_path)
    for hs in (ha, hb):
        for i, h in enumerate(hs):
            for attr, fn in damages(h).get(i, []):
                T.change(getattr(h, attr), fn)
    for x, y in zip(ha, hb):                      # damaged identically
        assert [T.read_or_none(p) for p in T.files_of(x)] == [T.read_or_none(p) for p in T.files_of(y)]
    return ha, hb, roots


def same_entries(PF, got, want):
    assert len(got) == len(want) == len(FILES)
    ok = []
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, Exception):
            assert type(g) is type(w), (i, g, w)
        else:
            assert isinstance(g, PF.ScrubReport) and dataclasses.asdict(g) == dataclasses.asdict(w), (i, g, w)
            ok.append(i)
    return ok


def same_files(ha, hb):
    for i, (x, y) in enumerate(zip(ha, hb)):
        for p, q in zip(T.files_of(x), T.files_of(y)):
            assert T.read_or_none(p) == T.read_or_none(q), (i, p)


@pytest.mark.parametrize("with_roots", [True, False])
def test_scrub_and_repair_with_locate_equal_the_loops(PF, tmp_path, with_roots):
    ha, hb, roots = damaged_store(PF, tmp_path)
    er = roots if with_roots else [None] * len(roots)
    got = PF.scrub_files(ha, er, locate=True)
    want = [h.scrub(expected_root=r, locate=True) for h, r in zip(hb, er)]
    assert same_entries(PF, got, want) == list(range(len(FILES)))
    same_files(ha, hb)
    # what the test set up did happen
    assert got[0].located_columns == [5] and got[1].located_columns == [9] and got[3].located_columns == []
    assert got[4].unlocatable_rows == 0 and len(got[4].located_columns) == (ha[4].encoded_size - ha[4].pre_encoded_size) // 2
    assert got[5].unlocatable_rows == 1 and got[12].unlocatable_rows == 1
    assert got[9].located_columns == [3, 4, 100] and got[9].noncanonical_columns == [100]
    got = PF.repair_files(ha, er, locate=True)
    want = T.loop_repair(PF, hb, er, True)
    mended = same_entries(PF, got, want)
    same_files(ha, hb)
    assert got[6].repaired_from.startswith("located") and got[7].repaired_from.startswith("located")
    assert got[5].repaired_from == "columns" and isinstance(got[12], PF.UnrecoverableError)
    # (12 always; without roots a damaged or missing raw file cannot vouch for a located repair: 14 and 19)
    assert len(mended) >= len(FILES) - (1 if with_roots else 3)
    again = PF.scrub_files([ha[i] for i in mended], [er[i] for i in mended], locate=True)
    for i, r in zip(mended, again):
        assert r.clean and r.located_columns == [] and r.unlocatable_rows == 0, (i, r)
        ha[i].verify_all_files_agree()


def test_a_store_without_trees_is_repaired_by_the_grouped_legs_alone(gpu, PF, tmp_path):
    """every `.portree` deleted, all damage locatable: scrub, ingest, locate and repair per staging group of
    files, and no per-file locate or repair region"""
    ha, _, roots = T.build_store(PF, tmp_path)
    plain = [i for i, f in enumerate(FILES) if not f[3]]
    hs, rs = [ha[i] for i in plain], [roots[i] for i in plain]
    for k, h in enumerate(hs):
        os.remove(h.merkle_tree_file_handle)
        if k % 3 != 2:
            T.change(h.encoded_file_handle, T.flip_elems(h, range(k % 5, k % 5 + 1 + k % 4), row=k % 2))
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = PF.repair_files(hs, rs, locate=True)
        stats = gpu.prof_stats()
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert [r.repaired_from for r in got] == ["located+columns+tree" if k % 3 != 2 else "located+tree" for k in range(len(hs))]
    assert [r.located_columns for r in got] == [list(range(k % 5, k % 5 + 1 + k % 4)) if k % 3 != 2 else [] for k in range(len(hs))]
    assert all(stats[name][1] >= 1 for name in GROUPED), sorted(stats)
    assert stats["pos_group_locate"][1] == 1 and stats["pos_group_repair"][1] == 1
    assert all(name.startswith(GROUPED) for name in stats), sorted(stats)
    for h, r in zip(hs, PF.scrub_files(hs, rs, locate=True)):
        assert r.clean and r.located_columns == []
        h.verify_all_files_agree()

