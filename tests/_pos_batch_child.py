"""Child process of test_gpu_pos_batch_audit.py: the cases of CHILD_CASES through
lcpc_pos_left_multiply_bytes_many under whatever LCPC_NO_MFMA this process was started with (the
library reads it once), the raw output words written one case after another to the file named in
argv[1].  Under LCPC_NO_MFMA=1 it also checks that no case names the matrix-core kernel."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcpc_proof_of_storage_amd as L  # noqa: E402
from lcpc_proof_of_storage_amd import pos  # noqa: E402

# (pre, rows, bytes cut from the last row, vectors): both sides of the dispatch boundary, the K step
# and the split boundaries, one chunk and one more, pack-first at pre = 24
CHILD_CASES = [(8, 9, 0, 5), (32, 513, 3, 17), (64, 1, 0, 1), (64, 7, 5, 2), (64, 9, 200, 3), (64, 512, 0, 16),
               (64, 513, 447, 17), (128, 511, 10, 17), (128, 17, 0, 4), (256, 1030, 1, 33), (24, 11, 4, 5)]


def inputs(case):
    pre, rows, cut, m = case
    rng = np.random.default_rng(7000 + 131 * pre + 7 * rows + m)
    data = rng.integers(0, 256, 7 * pre * rows - cut, dtype=np.uint8)
    return data, L.field_random(0, m * rows, 7000 + rows + m).reshape(m, rows)


def run_cases() -> bytes:
    out = []
    for case in CHILD_CASES:
        data, lefts = inputs(case)
        out.append(pos.left_multiply_unencoded_matrix_by_vectors(data, case[0], lefts).tobytes())
    return b"".join(out)


if __name__ == "__main__":
    assert L.device_count() > 0, "no HIP device"
    L.set_device(0)
    if os.environ.get("LCPC_NO_MFMA") == "1":
        assert all(pos.left_multiply_many_kernel(c[0], c[3]) != pos.LEFT_MANY_MFMA for c in CHILD_CASES)
    with open(sys.argv[1], "wb") as f:
        f.write(run_cases())
