"""Child process of test_gpu_pos_group_locate.py::test_a_recycled_pool_changes_nothing: a mixed queue A of
the grouped locate, then a queue B of other verdicts (forwards and backwards, so that every device block
comes back in a role that held other bytes), in one process whose pool may prefill every block
(LCPC_POOL_POISON).  Prints `digest <sha256 of everything B's calls returned>`."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from lcpc_proof_of_storage_amd import _native, pos  # noqa: E402
import test_gpu_pos_group_locate as T  # noqa: E402


def main():
    _native.load()
    a_files, a_knowns, _ = T.mixed_fleet(pos, _native, 120, seed=12)
    T.call(pos, a_files, a_knowns)
    files, knowns, _ = T.mixed_fleet(pos, _native, 120, seed=11)
    h = hashlib.sha256()
    for r in T.call(pos, files, knowns) + T.call(pos, files[::-1], knowns[::-1]):
        h.update(repr(r["status"]).encode())
        if not r["status"]:
            h.update(r["col_status"].tobytes() + r["row_status"].tobytes())
    print("digest " + h.hexdigest())


if __name__ == "__main__":
    main()
