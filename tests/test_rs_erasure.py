"""CPU: the host-only parts of Reed-Solomon erasure decoding (include/lcpc_mi.h, "R-S erasure
decoding, scrub, repair"; no counterpart in the reference).

* lcpc_rs_domain_points gives, for all five fields and every length 2 .. 64, the oracle's fft_io of
  the polynomial x -- position c of a codeword of f is f(points[c]) -- and the points are distinct;
* bad lengths give the FFTError codes of the transforms;
* the new symbols are declared, exported and bound, and the ABI version is 3;
* the argument rules of the compute entry points hold before any device is touched, and with no
  HIP device each of them fails with the no-device error (a child process that hides the devices,
  so the check also runs where a GPU is present).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")
FIELDS = [0, 1, 2, 3, 4]
NEW_SYMBOLS = ["lcpc_rs_domain_points", "lcpc_rs_erasure_decode_rows", "lcpc_pos_scrub_porenc",
               "lcpc_pos_repair_columns"]


@pytest.fixture(scope="module")
def native():
    from lcpc_proof_of_storage_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.run(["make", "-s", "-j8", "-C", PKG], check=True)
    N.load()
    return N


@pytest.fixture(scope="module")
def pos(native):
    from lcpc_proof_of_storage_amd import pos
    return pos


@pytest.mark.parametrize("fid", FIELDS)
def test_domain_points_are_the_encode_of_x(pos, oracle, fid):
    nl = oracle.limbs(fid)
    for log_n in range(1, 7):
        n = 1 << log_n
        x = oracle.to_mont(fid, [0, 1] + [0] * (n - 2))          # the polynomial x
        want = oracle.fft_io(fid, x).reshape(n, nl)
        got = pos.rs_domain_points(fid, n)
        assert got.shape == (n, nl)
        assert np.array_equal(got, want), (fid, n)
        # pairwise differences are non-zero: the points are n distinct field elements, all < p
        vals = oracle.from_mont(fid, got.reshape(-1))
        assert len(set(vals)) == n and max(vals) < oracle.modulus(fid)


def test_domain_points_length_one_and_bad_lengths(pos, oracle, native):
    from lcpc_proof_of_storage_amd import lcpc2d
    for fid in FIELDS:
        one = pos.rs_domain_points(fid, 1)           # fft_io of a length-1 input is the identity
        assert oracle.from_mont(fid, one.reshape(-1)) == [1]
        for bad in (0, 3, 6, 63):
            with pytest.raises(lcpc2d.FFTError) as e:
                pos.rs_domain_points(fid, bad)
            assert e.value.code == 20                # FFTError::NotPowerOfTwo
    # 2-adicity: S = 41 for Ft63, 40 for Ft127; nothing is written before the length check
    buf = np.zeros(4, np.uint64)
    lib = native.load()
    assert lib.lcpc_rs_domain_points(0, 1 << 42, buf.ctypes.data_as(native.u64p)) == 21   # FFTError::TooBig
    assert lib.lcpc_rs_domain_points(1, 1 << 41, buf.ctypes.data_as(native.u64p)) == 21
    assert lib.lcpc_rs_domain_points(7, 4, buf.ctypes.data_as(native.u64p)) == 30
    assert lib.lcpc_rs_domain_points(0, 4, None) == 30
    assert not buf.any()


def test_new_symbols_declared_exported_bound(native):
    import ctypes as C
    import re
    declared = set(native.header_symbols())
    raw = C.CDLL(native.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in native.SIGNATURES, s
    assert native.load().lcpc_abi_version() == 3
    text = open(native.HEADER_PATH).read()
    assert re.search(r"LCPC_ERR_UNRECOVERABLE\s*=\s*36\b", text)
    assert pos_unrecoverable() == 36


def pos_unrecoverable():
    from lcpc_proof_of_storage_amd import pos, pos_files
    assert pos.UNRECOVERABLE == pos_files.LCPC_ERR_UNRECOVERABLE
    return pos.UNRECOVERABLE


def test_argument_rules_hold_before_any_device(native):
    """index >= len, a duplicate, n_per_row outside [1, len): LCPC_ERR_INVALID_ARG (30); more
    erasures than len - n_per_row: LCPC_ERR_UNRECOVERABLE (36); a bad length: the FFTError codes."""
    lib, u64p = native.load(), native.u64p
    rows = np.zeros(16, np.uint64)
    keep = rows.copy()

    def call(fid, length, npr, erased):
        e = np.asarray(erased, np.uint64)
        return lib.lcpc_rs_erasure_decode_rows(fid, rows.ctypes.data_as(u64p), 1, length, npr,
                                               e.ctypes.data_as(u64p) if e.size else None, e.size)
    assert call(0, 16, 5, [16]) == 30
    assert call(0, 16, 5, [3, 3]) == 30
    assert call(0, 16, 0, []) == 30
    assert call(0, 16, 16, []) == 30
    assert call(0, 16, 5, list(range(12))) == 36
    assert call(0, 12, 5, []) == 20
    assert call(9, 16, 5, []) == 30
    assert np.array_equal(rows, keep)
    img = np.zeros(4 * 2 * 8, np.uint8)
    out = np.zeros(4 * 8, np.uint8)
    u8p = native.u8p

    def rep(pre, enc, bad):
        b = np.asarray(bad, np.uint64)
        return lib.lcpc_pos_repair_columns(img.ctypes.data_as(u8p), pre, enc, 1, 2, b.ctypes.data_as(u64p) if b.size
                                           else None, b.size, out.ctypes.data_as(u8p), None, None)
    assert rep(2, 4, [4]) == 30
    assert rep(2, 4, [1, 1]) == 30
    assert rep(2, 4, [0, 1, 2]) == 36
    assert rep(4, 4, []) == 30
    assert rep(2, 6, []) == 30
    st = np.zeros(4, np.uint8)
    assert lib.lcpc_pos_scrub_porenc(img.ctypes.data_as(u8p), 6, 1, 2, out.ctypes.data_as(u8p), None,
                                     st.ctypes.data_as(u8p), None) == 30
    assert lib.lcpc_pos_scrub_porenc(img.ctypes.data_as(u8p), 4, 3, 2, out.ctypes.data_as(u8p), None,
                                     st.ctypes.data_as(u8p), None) == 30


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from lcpc_proof_of_storage_amd import _native as N, lcpc2d, pos, pos_files
assert lcpc2d.device_count() == 0, "the child must see no device"
img = np.zeros(4 * 2 * 8, np.uint8)
f = open(sys.argv[2], "w+b")
f.write(img.tobytes())
f.flush()
r = pos_files.EncodedFileReader.new_ligero(f, 2, 4, 1, 2)
tree = pos_files.MerkleTree(np.zeros((7, 32), np.uint8))
calls = {
    "erasure_decode_rows": lambda: pos.erasure_decode_rows(0, np.zeros((1, 4, 1), np.uint64), 2, [1]),
    "erasure_decode_rows (check only)": lambda: pos.erasure_decode_rows(1, np.zeros((2, 8, 2), np.uint64), 3, []),
    "find_damaged_columns": lambda: r.find_damaged_columns(tree),
    "repair_columns": lambda: r.repair_columns([1]),
    "decode_with_erasures": lambda: r.decode_with_erasures([0, 3]),
}
for name, fn in calls.items():
    try:
        fn()
    except lcpc2d.DeviceError as e:
        assert e.code == 33, (name, e.code)          # LCPC_ERR_NO_DEVICE
        assert "no HIP device" in str(e), (name, str(e))
    else:
        raise SystemExit(name + ": no error without a device")
pts = pos.rs_domain_points(0, 8)                     # host only: works with no device
assert pts.shape == (8, 1) and len(set(int(v) for v in pts.reshape(-1))) == 8
print("child ok")
"""


def test_compute_entry_points_fail_loudly_without_device(native, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", _CHILD, ROOT, str(tmp_path / "x.porenc")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
