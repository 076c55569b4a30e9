"""CPU: the symbols and the argument checks of the grouped locate of stored files (DESIGN §5m,
lcpc_pos_locate_files_grouped).  Every argument error comes before any device work and before any output
byte is written, so no device is needed: the outputs and every job's status field are prefilled and must
come back as they were."""
import ctypes as C

import numpy as np
import pytest

INVALID_ARG = 30
FILL, STATUS_FILL, COUNT_FILL = 0x5C, 77, 12345


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


def test_symbols(native):
    from lcpc_proof_of_storage_amd import pos
    lib = native.load()
    assert hasattr(lib, "lcpc_pos_locate_files_grouped")
    assert "lcpc_pos_locate_files_grouped" in native.SIGNATURES
    assert C.sizeof(native.PosLocateJob) == 13 * 8          # twelve words and the status, padded
    assert [n for n, _ in native.PosLocateJob._fields_] == [
        "porenc", "pre", "enc", "rows_written", "row_capacity", "known_bad", "n_known", "col_status", "row_status",
        "n_bad_cols", "n_dirty_rows", "n_unlocatable_rows", "status"]
    assert callable(pos.locate_files_grouped)
    assert (pos.LOCATE_MAX_ENC, pos.LOCATE_LAUNCHES_PER_GROUP, pos.LOCATE_ROW_NOT_EVALUATED) == (1024, 4, 0xFF)


class Queue:
    """three well-formed jobs with prefilled outputs; break(j, **fields) makes job j ill-formed"""

    def __init__(self, native):
        self.N = native
        self.keep, self.jobs = [], []
        for pre, enc, rows, known in ((8, 16, 5, [3]), (24, 32, 0, []), (100, 256, 9, [0, 255, 7])):
            cap = 2 * rows + 3
            img = np.zeros(enc * cap, np.uint64)
            kb = np.asarray(known, np.uint64)
            cs, rs = np.full(enc, FILL, np.uint8), np.full(max(rows, 1), FILL, np.uint8)
            self.keep.append((img, kb, cs, rs))
            self.jobs.append(dict(porenc=img.ctypes.data if rows else None, pre=pre, enc=enc, rows_written=rows,
                                  row_capacity=cap, known_bad=kb.ctypes.data if kb.size else None, n_known=kb.size,
                                  col_status=cs.ctypes.data, row_status=rs.ctypes.data, n_bad_cols=COUNT_FILL,
                                  n_dirty_rows=COUNT_FILL, n_unlocatable_rows=COUNT_FILL, status=STATUS_FILL))

    def run(self):
        arr = (self.N.PosLocateJob * len(self.jobs))(*[self.N.PosLocateJob(**j) for j in self.jobs])
        st = self.N.load().lcpc_pos_locate_files_grouped(arr, len(self.jobs))
        return st, arr

    def untouched(self, arr):
        for a, (_, _, cs, rs) in zip(arr, self.keep):
            assert a.status == STATUS_FILL
            assert (a.n_bad_cols, a.n_dirty_rows, a.n_unlocatable_rows) == (COUNT_FILL,) * 3
            assert (cs == FILL).all() and (rs == FILL).all()


def test_null_queue_and_no_jobs(native):
    lib = native.load()
    assert lib.lcpc_pos_locate_files_grouped(None, 3) == INVALID_ARG
    q = Queue(native)
    arr = (native.PosLocateJob * 3)(*[native.PosLocateJob(**j) for j in q.jobs])
    assert lib.lcpc_pos_locate_files_grouped(arr, 0) == INVALID_ARG
    q.untouched(arr)


BREAKS = {
    "null col_status": dict(col_status=None),
    "index >= enc": "index",
    "duplicate index": "duplicate",
    "rows_written > row_capacity": dict(rows_written=22),
    "enc == pre": dict(pre=256),
    "enc < pre": dict(pre=300),
    "enc no power of two": dict(enc=255),
    "pre == 0": dict(pre=0),
    "no image": dict(porenc=None),
    "no list": dict(known_bad=None),
}


@pytest.mark.parametrize("what", sorted(BREAKS))
def test_an_ill_formed_last_job_fails_the_call_before_anything_is_written(native, what):
    """the error is in the LAST job: the jobs before it are well-formed and must not have been answered"""
    q = Queue(native)
    b = BREAKS[what]
    if b == "index":
        bad = np.asarray([0, 256, 7], np.uint64)
        q.keep.append(bad)
        b = dict(known_bad=bad.ctypes.data)
    elif b == "duplicate":
        bad = np.asarray([7, 255, 7], np.uint64)
        q.keep.append(bad)
        b = dict(known_bad=bad.ctypes.data)
    q.jobs[2].update(b)
    st, arr = q.run()
    assert st == INVALID_ARG, what
    q.untouched(arr)
    assert b"" != native.load().lcpc_last_error()
