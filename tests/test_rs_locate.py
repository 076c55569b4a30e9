"""CPU: Reed-Solomon error location by syndromes (include/lcpc_mi.h, "R-S error location by
syndromes"; no counterpart in the reference) -- the parts that need no device.

* the Python reference of the GPU tests (rs_locate_ref.py) against brute force: for all five fields
  at (n_per_row, len) in {(2,4), (5,16), (16,32), (16,64)} it returns exactly the injected set for
  every t <= N / 2, N = len - n_per_row - n_erased, with and without erasures, and status 2 for the
  seeded inputs with t = N / 2 + 1 (seeds: SEED_BASE + 1000 fid + len + 7 n_erased, every one of
  them checked here);
* Horner evaluation and the oracle's fft_io give the reference the same roots;
* the new symbols are declared, exported and bound, and the ABI version is still 3;
* the argument rules hold before a device is touched;
* with the devices hidden (a child process) each compute entry fails with the no-device error;
* lcpc_rs_locate_max_errors(f) >= 256 for every field.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rs_locate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lcpc_proof_of_storage_amd")
FIELDS = [0, 1, 2, 3, 4]
SHAPES = [(2, 4), (5, 16), (16, 32), (16, 64)]
SEED_BASE = 0xB3A5
NEW_SYMBOLS = ["lcpc_rs_locate_max_errors", "lcpc_rs_locate_errors_rows", "lcpc_rs_decode_rows",
               "lcpc_pos_locate_porenc"]


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


def erasure_counts(npr, length):
    m = length - npr
    return sorted({0, 1, m // 2, m - 2})


@pytest.mark.parametrize("npr,length", SHAPES)
@pytest.mark.parametrize("fid", FIELDS)
def test_reference_returns_the_injected_set(pos, oracle, fid, npr, length):
    cw = R.codewords(fid, npr, length, 8)
    r = 0
    for n_erased in erasure_counts(npr, length):
        rng = np.random.default_rng(SEED_BASE + 1000 * fid + length + 7 * n_erased)
        erased = sorted(int(c) for c in rng.permutation(length)[:n_erased])
        avail = [c for c in range(length) if c not in erased]
        loc = R.Locator(pos, fid, length, npr, erased)
        N = length - npr - n_erased
        assert loc.N == N
        for t in range(0, N // 2 + 1):
            for pattern in range(4):
                where = R.error_positions(avail, t, pattern, rng)
                row = R.damage(fid, cw[r % 8], where, erased, rng, plus_one=(r % 3 == 0))
                r += 1
                want = (1, t, sorted(where)) if t else (0, 0, [])
                assert loc.locate(row) == want, (fid, npr, length, n_erased, t, pattern)
        # beyond the radius: not locatable (the seeds above are chosen so, and all are checked)
        t = N // 2 + 1
        if t <= len(avail):
            for pattern in range(4):
                where = R.error_positions(avail, t, pattern, rng)
                row = R.damage(fid, cw[r % 8], where, erased, rng)
                r += 1
                assert loc.locate(row)[0] == 2, (fid, npr, length, n_erased, pattern)


def test_reference_roots_by_fft_equal_horner(pos, oracle):
    fid, npr, length = 1, 16, 64
    cw = R.codewords(fid, npr, length, 8)
    rng = np.random.default_rng(SEED_BASE)
    erased = [3, 40]
    avail = [c for c in range(length) if c not in erased]
    a = R.Locator(pos, fid, length, npr, erased, roots_by="horner")
    b = R.Locator(pos, fid, length, npr, erased, roots_by="fft")
    for t in (1, 7, 23, 24):
        row = R.damage(fid, cw[t % 8], R.error_positions(avail, t, 3, rng), erased, rng)
        assert a.locate(row) == b.locate(row)


def test_reference_cap(pos, oracle):
    fid, npr, length = 0, 16, 64
    cw = R.codewords(fid, npr, length, 8)
    rng = np.random.default_rng(SEED_BASE + 1)
    where = R.error_positions(list(range(length)), 5, 3, rng)
    row = R.damage(fid, cw[0], where, [], rng)
    assert R.Locator(pos, fid, length, npr, [], max_errors=5).locate(row) == (1, 5, where)
    assert R.Locator(pos, fid, length, npr, [], max_errors=4).locate(row)[0] == 2


def test_new_symbols_declared_exported_bound(native):
    import ctypes as C
    declared = set(native.header_symbols())
    raw = C.CDLL(native.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(raw, s), s
        assert s in native.SIGNATURES, s
    assert native.load().lcpc_abi_version() == 3
    assert "additive" in open(native.HEADER_PATH).read()


@pytest.mark.parametrize("fid", FIELDS)
def test_max_errors_at_least_256(native, pos, fid):
    assert native.load().lcpc_rs_locate_max_errors(fid) >= 256
    assert pos.rs_locate_max_errors(fid) == native.load().lcpc_rs_locate_max_errors(fid)
    assert native.load().lcpc_rs_locate_max_errors(9) == 0


def test_argument_rules_hold_before_any_device(native):
    """index >= len, a duplicate, n_per_row outside [1, len), a null rows / row_status: INVALID_ARG (30);
    more erasures than len - n_per_row: UNRECOVERABLE (36); a bad length: the FFTError codes."""
    lib, u64p, u8p = native.load(), native.u64p, native.u8p
    rows = np.zeros(16, np.uint64)
    keep = rows.copy()
    status = np.zeros(1, np.uint8)

    def locate(fid, length, npr, erased, rows_p=None, status_p=None):
        e = np.asarray(erased, np.uint64)
        return lib.lcpc_rs_locate_errors_rows(fid, rows_p or rows.ctypes.data_as(u64p), 1, length, npr,
                                              e.ctypes.data_as(u64p) if e.size else None, e.size,
                                              status_p or status.ctypes.data_as(u8p), None, None, None)

    def decode(fid, length, npr, erased):
        e = np.asarray(erased, np.uint64)
        return lib.lcpc_rs_decode_rows(fid, rows.ctypes.data_as(u64p), 1, length, npr,
                                       e.ctypes.data_as(u64p) if e.size else None, e.size, None)
    for call in (locate, decode):
        assert call(0, 16, 5, [16]) == 30
        assert call(0, 16, 5, [3, 3]) == 30
        assert call(0, 16, 0, []) == 30
        assert call(0, 16, 16, []) == 30
        assert call(0, 16, 5, list(range(12))) == 36
        assert call(0, 12, 5, []) == 20
        assert call(9, 16, 5, []) == 30
    assert lib.lcpc_rs_locate_errors_rows(0, None, 1, 16, 5, None, 0, status.ctypes.data_as(u8p), None, None,
                                          None) == 30
    assert lib.lcpc_rs_locate_errors_rows(0, rows.ctypes.data_as(u64p), 1, 16, 5, None, 0, None, None, None,
                                          None) == 30
    assert lib.lcpc_rs_locate_errors_rows(0, None, 0, 16, 5, None, 0, None, None, None, None) == 0   # no rows
    assert lib.lcpc_rs_decode_rows(0, None, 0, 16, 5, None, 0, None) == 0
    assert np.array_equal(rows, keep) and not status.any()
    img = np.zeros(4 * 2 * 8, np.uint8)
    st = np.zeros(4, np.uint8)

    def loc(pre, enc, known, rows_written=1, cap=2, st_p=None):
        b = np.asarray(known, np.uint64)
        return lib.lcpc_pos_locate_porenc(img.ctypes.data_as(u8p), pre, enc, rows_written, cap,
                                          b.ctypes.data_as(u64p) if b.size else None, b.size,
                                          st_p or st.ctypes.data_as(u8p), None, None, None)
    assert loc(2, 4, [4]) == 30
    assert loc(2, 4, [1, 1]) == 30
    assert loc(2, 4, [0, 1, 2]) == 36
    assert loc(4, 4, []) == 30
    assert loc(2, 6, []) == 30
    assert loc(2, 4, [], rows_written=3) == 30
    assert lib.lcpc_pos_locate_porenc(img.ctypes.data_as(u8p), 2, 4, 1, 2, None, 0, None, None, None, None) == 30
    assert not st.any()


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
calls = {
    "locate_errors_rows": lambda: pos.locate_errors_rows(0, np.zeros((1, 4, 1), np.uint64), 2, [1]),
    "locate_errors_rows (no erasures)": lambda: pos.locate_errors_rows(1, np.zeros((2, 8, 2), np.uint64), 3),
    "decode_rows": lambda: pos.decode_rows(2, np.zeros((1, 4, 3), np.uint64), 2, [0]),
    "locate_damaged_columns": lambda: r.locate_damaged_columns(),
    "locate_damaged_columns (known)": lambda: r.locate_damaged_columns([2]),
}
for name, fn in calls.items():
    try:
        fn()
    except lcpc2d.DeviceError as e:
        assert e.code == 33, (name, e.code)          # LCPC_ERR_NO_DEVICE
        assert "no HIP device" in str(e), (name, str(e))
    else:
        raise SystemExit(name + ": no error without a device")
assert pos.rs_locate_max_errors(0) >= 256            # host only: works with no device
print("child ok")
"""


def test_compute_entry_points_fail_loudly_without_device(native, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", _CHILD, ROOT, str(tmp_path / "x.porenc")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_scrub_report_defaults_are_unchanged():
    from lcpc_proof_of_storage_amd import pos_files as PF
    rep = PF.ScrubReport(bad_columns=[], noncanonical_columns=[], tree_consistent=True, root_ok=None, raw_ok=True)
    assert rep.located_columns is None and rep.unlocatable_rows is None and rep.clean
