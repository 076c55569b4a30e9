"""The persistent encode passes (csrc/ntt_v2.hpp, k_pass_a_loop / k_pass_b_loop) at the edges of
their tile loop, against oracle.fft_io.  The default build loops pass A and keeps pass B on the
one-tile kernel; a -DLCPC_NTT_PERSIST_B=1 build loops both, and these cases hold for it as they
stand (pass B has the same groups per row at both sizes).

A workgroup walks tiles blockIdx.x, blockIdx.x + grid, ...; it stages its twiddles once, issues the
next tile's round-0 loads before the current tile's last round, and pass A keeps its inter-pass
twiddles in registers when the grid is a multiple of the column groups per row.  What can go wrong
is therefore a matter of (tiles, grid): a workgroup with one tile only, a last tile without a
successor, a grid below / equal to / not a multiple of the groups, and the predicates of a
prefetched tile (n_valid inside it).  LCPC_NTT_PERSIST_GRID is read when a plan is made, so every
case makes its encoding (or its selftest plan) under the grid it wants; few rows then suffice.

Ft127 2^16 is the flagship instantiation (<8,3,8>, 32 groups per row in both passes), 2^13 the
smallest four-step row (4 groups per row).  The other fields keep the one-tile kernels under the
same launcher; their cases show the override leaves them alone.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FT63, FT127, FT255 = 0, 1, 3
GRID_ENV = "LCPC_NTT_PERSIST_GRID"
SENTINEL = np.uint64(0xA5C3A5C3A5C3A5C3)
GRIDS = [1, 5, 32, 33, 96]
MAX_ROWS = {16: 25, 13: 7}


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv(GRID_ENV, raising=False)
    else:
        monkeypatch.setenv(GRID_ENV, str(grid))


def _canonical(oracle, fid, a):
    out = np.zeros_like(a)
    oracle.lib().of_to_canonical(fid, oracle.p64(a), oracle.p64(out), a.size // oracle.limbs(fid))
    return out


class _Refs:
    """Rows of random coefficients and their transforms, computed once per (field, log_n, n_valid)."""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def get(self, fid, log_n, nv, rows):
        key = (fid, log_n, nv)
        have = self.cache.get(key)
        if have is None or have[0].shape[0] < rows:
            n, nl = 1 << log_n, self.oracle.limbs(fid)
            coeffs = self.oracle.random_coeffs(fid, rows * nv, seed_u64=0x9E50000 + 4096 * fid + 64 * log_n + nv % 61)
            coeffs = coeffs.reshape(rows, nv * nl)
            want = np.zeros((rows, n * nl), np.uint64)
            for r in range(rows):
                row = np.zeros(n * nl, np.uint64)
                row[: nv * nl] = coeffs[r]
                want[r] = self.oracle.fft_io(fid, row)
            have = (coeffs, want)
            self.cache[key] = have
        coeffs, want = have
        coeffs.setflags(write=False)
        want.setflags(write=False)
        return coeffs[:rows], want[:rows]


@pytest.fixture(scope="module")
def refs(oracle):
    return _Refs(oracle)


def _encode_rows_device(gpu, hipmem, fid, log_n, coeffs, nv, ss):
    """encode_rows_device of coeffs' rows (stride ss) into a destination of stride n + 3 with a
    tail of four more strides; returns the whole destination buffer as (rows + 4, ds * nl)."""
    rows, n, nl = coeffs.shape[0], 1 << log_n, coeffs.shape[1] // nv
    ds = n + 3
    src = np.full((rows, ss * nl), SENTINEL, np.uint64)
    src[:, : nv * nl] = coeffs
    dst = np.full((rows + 4, ds * nl), SENTINEL, np.uint64)
    enc = gpu.RsEncoding.new(fid, n // 2, n, 4, 1)
    d_src, d_dst = hipmem.to_device(src), hipmem.to_device(dst)
    try:
        enc.encode_rows_device(d_src, ss, nv, d_dst, ds, rows)
        hipmem.to_host(d_dst, dst)
        back = hipmem.to_host(d_src, np.zeros_like(src))
    finally:
        hipmem.free(d_src)
        hipmem.free(d_dst)
    assert np.array_equal(back, src), "the source was written"
    return dst


@pytest.mark.parametrize("rows", [1, 2, 3, 7])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("log_n", [16, 13])
def test_loop_edges(gpu, oracle, hipmem, refs, monkeypatch, log_n, grid, rows):
    """Rate-1/2 rows through encode_rows_device at forced grids: one workgroup walks everything (1),
    fewer workgroups than column groups (5: the per-tile inter-pass twiddles), exactly the groups
    (32), not a multiple of them (33), more workgroups than tiles (96 with one or two rows at 2^16:
    the launcher clamps the grid to the tiles, so every workgroup runs the loop body exactly once).
    With 1, 2, 3 and 7 rows (32 tiles per row at 2^16, 4 at 2^13) the tiles fall below, on, one past
    and raggedly past the grid."""
    _set_grid(monkeypatch, grid)
    n, nl = 1 << log_n, oracle.limbs(FT127)
    nv = n // 2
    coeffs, want = refs.get(FT127, log_n, nv, MAX_ROWS[log_n])
    dst = _encode_rows_device(gpu, hipmem, FT127, log_n, coeffs[:rows], nv, nv)
    assert np.array_equal(dst[:rows, : n * nl], want[:rows])
    assert (dst[:rows, n * nl:] == SENTINEL).all(), "a row's gap was written"
    assert (dst[rows:] == SENTINEL).all(), "the tail past the last row was written"


def test_default_grid_more_tiles_than_workgroups(gpu, oracle, hipmem, refs, monkeypatch):
    """25 rows of 2^16 points are 800 tiles per pass, more than the blocks an MI355X holds at three
    per CU: at the plan's own grid some workgroups take a second tile and most do not."""
    _set_grid(monkeypatch, None)
    log_n, rows = 16, 25
    n, nl = 1 << log_n, oracle.limbs(FT127)
    coeffs, want = refs.get(FT127, log_n, n // 2, rows)
    dst = _encode_rows_device(gpu, hipmem, FT127, log_n, coeffs, n // 2, n // 2)
    assert np.array_equal(dst[:rows, : n * nl], want)
    assert (dst[:rows, n * nl:] == SENTINEL).all() and (dst[rows:] == SENTINEL).all()


def _selftest(gpu, oracle, fid, log_n, coeffs, want, nv, canon, with_copy):
    """ntt_rows through the selftest entry: src_stride and copy_stride above n_valid, dst_stride
    above n; src holds the sentinel past n_valid (it must read as zero), dst and copy start as the
    sentinel and must keep it wherever the transform does not write.  The entry moves whole
    strides, so the tail past the last row is the last row's gap: 67 elements of copy (more than
    a wave's 64 lanes of one column segment) and 7 of dst."""
    rows, n, nl = coeffs.shape[0], 1 << log_n, oracle.limbs(fid)
    ss, ds, cs = nv + 5, n + 7, nv + 67
    src = np.full((rows, ss * nl), SENTINEL, np.uint64)
    src[:, : nv * nl] = coeffs
    dst = np.full((rows, ds * nl), SENTINEL, np.uint64)
    cp = np.full((rows, cs * nl), SENTINEL, np.uint64) if with_copy else None
    gpu.selftest_ntt_rows(fid, log_n, src, nv, dst, n_rows=rows, src_stride=ss, dst_stride=ds, copy=cp,
                          copy_stride=cs if with_copy else None, canon=canon)
    ref = _canonical(oracle, fid, np.ascontiguousarray(want).reshape(-1)).reshape(rows, -1) if canon else want
    assert np.array_equal(dst[:, : n * nl], ref), "transform"
    assert (dst[:, n * nl:] == SENTINEL).all(), "dst written past a row"
    if with_copy:
        assert np.array_equal(cp[:, : nv * nl], coeffs), "coefficient copy"
        assert (cp[:, nv * nl:] == SENTINEL).all(), "copy written past n_valid"


def _nv_cases(n):
    return [1, n // 2 - 1, n // 2, n // 2 + 1, n]


@pytest.mark.parametrize("canon", [False, True], ids=["mont", "canon"])
@pytest.mark.parametrize("grid", [5, 33, None])
@pytest.mark.parametrize("which", range(5), ids=["nv1", "half-1", "half", "half+1", "full"])
def test_prefetch_predicates(gpu, oracle, refs, monkeypatch, which, grid, canon):
    """n_valid at 1, n/2 - 1, n/2 (the half-zero first stage), n/2 + 1 and n (the general one): the
    ragged end lies inside a prefetched tile, every stride exceeds its row, three rows so that at
    grids 5 and 33 every workgroup prefetches across a row boundary.  The fused coefficient copy
    rides on the Montgomery runs, the canonical runs go without it."""
    _set_grid(monkeypatch, grid)
    log_n = 16
    nv = _nv_cases(1 << log_n)[which]
    coeffs, want = refs.get(FT127, log_n, nv, 3)
    _selftest(gpu, oracle, FT127, log_n, coeffs, want, nv, canon, with_copy=not canon)


@pytest.mark.parametrize("which", [1, 3], ids=["half-1", "half+1"])
def test_prefetch_predicates_smallest_row(gpu, oracle, refs, monkeypatch, which):
    """The same at 2^13 points (64-point columns, 4 groups per row), seven rows on three workgroups."""
    _set_grid(monkeypatch, 3)
    log_n = 13
    nv = _nv_cases(1 << log_n)[which]
    coeffs, want = refs.get(FT127, log_n, nv, 7)
    _selftest(gpu, oracle, FT127, log_n, coeffs, want, nv, True, with_copy=True)


@pytest.mark.parametrize("grid", [5, 33, None])
def test_commit_device_with_copy(gpu, oracle, hipmem, monkeypatch, grid):
    """commit_device: canonical output and the fused coefficient copy together, a ragged last row
    (its n_valid is the row's, but the matrix ends inside it); the commitment equals the oracle's
    and lcpc_commit_copy_coeffs returns the input."""
    _set_grid(monkeypatch, grid)
    n_per_row, n_cols = 1 << 15, 1 << 16
    length = 6 * n_per_row + 77
    coeffs = oracle.ChaCha(seed_u64=0x9E5C0).field_random(FT127, length)
    g_enc = gpu.RsEncoding.new(FT127, n_per_row, n_cols, 16, 2)
    o = oracle.Commit(oracle.Encoding.ligero(FT127, n_per_row, n_cols, 16, 2), coeffs)
    d = hipmem.to_device(coeffs)
    try:
        g = gpu.LcCommit.commit_device(d, length, g_enc)
        assert np.array_equal(g.coeffs.reshape(-1), o.coeffs)
        assert np.array_equal(g.comm.reshape(-1), o.comm)
        assert g.get_root() == o.root()
        assert np.array_equal(hipmem.to_host(d, np.zeros_like(coeffs)), coeffs)
        del g
    finally:
        hipmem.free(d)


@pytest.mark.parametrize("grid", [1, 33])
@pytest.mark.parametrize("fid,log_n", [(FT63, 15), (FT255, 13)], ids=["Ft63-2p15", "Ft255-2p13"])
def test_other_fields_under_the_launcher(gpu, oracle, refs, monkeypatch, fid, log_n, grid):
    """Ft63 at the proof-of-storage row (the <8,5> pass A) and a 32-byte field at the smallest
    four-step row: they run the one-tile kernels, whatever grid the environment names."""
    _set_grid(monkeypatch, grid)
    nv = (1 << log_n) // 2
    coeffs, want = refs.get(fid, log_n, nv, 3)
    _selftest(gpu, oracle, fid, log_n, coeffs, want, nv, False, with_copy=True)
    _selftest(gpu, oracle, fid, log_n, coeffs, want, nv, True, with_copy=False)
