"""Child process of test_gpu_collapse_many.py: the six Ft127 cases of CHILD_CASES through
lcpc_collapse_columns_many under whatever LCPC_NO_MFMA this process was started with (the library
reads it once), the raw output words written one case after another to the file named in argv[1]."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcpc_proof_of_storage_amd as L  # noqa: E402

FID = 1
# (n_tensors, n_rows, n_per_row): ragged and aligned shapes, one and several chunks and row splits
CHILD_CASES = [(1, 17, 65), (5, 513, 255), (8, 512, 256), (9, 1025, 63), (17, 16, 257), (65, 5, 64)]


def inputs(case):
    n_t, n_rows, n_per_row = case
    seed = 9000 + 131 * n_t + 7 * n_rows + n_per_row
    return (L.field_random(FID, n_rows * n_per_row, seed),
            L.field_random(FID, n_t * n_rows, seed + 1).reshape(n_t, n_rows, -1))


def run_cases() -> bytes:
    out = []
    for case in CHILD_CASES:
        coeffs, tens = inputs(case)
        out.append(L.collapse_columns_many(FID, coeffs, tens, case[1], case[2]).tobytes())
    return b"".join(out)


if __name__ == "__main__":
    assert L.device_count() > 0, "no HIP device"
    L.set_device(0)
    with open(sys.argv[1], "wb") as f:
        f.write(run_cases())
