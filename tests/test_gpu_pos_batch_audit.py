"""GPU: batched audits of a stored file -- lcpc_pos_left_multiply_bytes_many (the VALU and the
matrix-core kernel of csrc/pos_eval.hip / pos_eval_mfma.hpp), lcpc_selftest_recombine63, and the
protocol on a FileHandler.  The reference is Python integers (tests/pos_batch_ref.py, update_ref);
all comparisons are exact."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pos_batch_ref as B
import update_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FT63 = 0
COLUMN_EVAL = 12
PACK, VALU, MFMA = 0, 1, 2
MFMA_MIN_PRE = 64      # one wave of the matrix-core kernel covers 64 columns
MFMA_MIN_VECS = 16     # the adoption measurement
VALU_CHUNK, MFMA_CHUNK = 4, 16
ROWS = (1, 7, 8, 9, 16, 17, 511, 512, 513)
VECS = (1, 2, 3, VALU_CHUNK, VALU_CHUNK + 1, MFMA_CHUNK, 17)
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    return N.load()


def expected_kernel(pre, m):
    if pre < 8 or pre & (pre - 1):
        return PACK
    return MFMA if pre >= MFMA_MIN_PRE and m >= MFMA_MIN_VECS else VALU


def reference(data: bytes, pre: int, lefts) -> np.ndarray:
    """(m, pre) words of sum_r left[r] M[r][c] / R mod p in Python integers"""
    el = R.pack7(data)
    rows = -(-len(el) // pre)
    el += [0] * (rows * pre - len(el))
    M = np.array(el, dtype=object).reshape(rows, pre)
    Lm = np.array([[int(v) for v in row] for row in lefts], dtype=object)
    out = Lm.dot(M)
    return np.array([[int(v) * B.RINV % B.P for v in row] for row in out], dtype=np.uint64)


def odd_address(data: np.ndarray) -> np.ndarray:
    buf = np.zeros(data.size + 17, np.uint8)
    start = 1 if buf.ctypes.data % 2 == 0 else 2
    view = buf[start:start + data.size]
    view[:] = data
    assert view.ctypes.data % 2 == 1
    return view


def many_device(native, hipmem, data: np.ndarray, pre: int, lefts: np.ndarray) -> np.ndarray:
    """the device entry from an image at dev + 8 (8-byte aligned only)"""
    m, rows = lefts.shape
    dev = hipmem.to_device(np.concatenate([np.zeros(8, np.uint8), data]))
    out = np.zeros((m, pre), np.uint64)
    lv = np.ascontiguousarray(lefts)
    try:
        st = native.lcpc_pos_left_multiply_bytes_many_device(dev + 8, data.size, pre, lv.ctypes.data_as(u64p), m, rows,
                                                             out.ctypes.data_as(u64p))
    finally:
        hipmem.free(dev)
    assert st == 0
    return out


@pytest.mark.parametrize("pre", [8, 16, 32, 64, 128])
def test_many_vectors_against_python_integers(gpu, pos, native, hipmem, pre):
    """Every row count around the K step (8) and the split bound (512), every vector count around
    the two kernels' chunks, whole files and files that end mid-element and mid-row, host bytes at
    an odd address; the kernel that ran is the one the shape is meant to exercise."""
    rng = np.random.default_rng(100 + pre)
    cuts = (0, 3, 7 * (pre // 2) + 2)
    for i, rows in enumerate(ROWS):
        cut = cuts[i % 3]
        data = odd_address(rng.integers(0, 256, 7 * pre * rows - cut, dtype=np.uint8))
        lefts = gpu.field_random(FT63, max(VECS) * rows, 900 + pre + rows).reshape(max(VECS), rows)
        want = reference(data.tobytes(), pre, lefts)
        for m in VECS:
            assert pos.left_multiply_many_kernel(pre, m) == expected_kernel(pre, m), (pre, m)
            got = pos.left_multiply_unencoded_matrix_by_vectors(data, pre, lefts[:m])
            assert np.array_equal(got, want[:m]), (pre, rows, cut, m)
        if rows in (9, 513):
            for m in (3, 17):
                assert np.array_equal(many_device(native, hipmem, data, pre, lefts[:m]), want[:m]), (pre, rows, m)
    # m = 1 is the single entry's vector, word for word
    one = pos.left_multiply_unencoded_matrix_by_vector(data.tobytes(), pre, lefts[0])
    assert np.array_equal(one.reshape(-1), want[0])


FILL = {0xff: (1 << 56) - 1, 0x00: 0, 0x80: 0x80808080808080, 0x7f: 0x7f7f7f7f7f7f7f}


@pytest.mark.parametrize("fill", sorted(FILL))
def test_extreme_images_at_512_rows(gpu, pos, fill):
    """512 rows x pre 64 (one split of the matrix-core kernel at its row bound) of one byte value
    against vectors of p - 1, 1, 0, R mod p and 12 of random words (16: the matrix-core kernel)."""
    pre, rows = 64, 512
    rnd = gpu.field_random(FT63, 12 * rows, 11).reshape(12, rows)
    lefts = np.concatenate([np.stack([np.full(rows, v, np.uint64) for v in (B.P - 1, 1, 0, B.R % B.P)]), rnd])
    assert pos.left_multiply_many_kernel(pre, len(lefts)) == MFMA
    got = pos.left_multiply_unencoded_matrix_by_vectors(np.full(7 * pre * rows, fill, np.uint8), pre, lefts)
    for t in range(len(lefts)):
        want = sum(int(v) for v in lefts[t]) * FILL[fill] * B.RINV % B.P
        assert [int(v) for v in got[t]] == [want] * pre, (fill, t)


def test_same_sign_accumulators(gpu, pos):
    """For each digit position u, an image whose bytes give every product in accumulator u one sign
    (and its mirror), 512 rows x pre 64: the exact |Y[u]| (Python integers) is below the kernel's
    bound and at least half of what the position can reach."""
    pre, rows = 64, 512
    assert pos.left_multiply_many_kernel(pre, MFMA_MIN_VECS) == MFMA
    for u in range(8):
        for mirror in (False, True):
            left, elems = B.same_sign_rows(u, rows, 300 + u, tries=16, mirror=mirror)
            Y = B.accumulators(left, elems)
            frac = abs(Y[u]) / B.reach(u)
            print(f"same sign u={u} mirror={mirror}: |Y| = 2^{np.log2(abs(Y[u])):.2f}, {frac:.3f} of the reach, "
                  f"{abs(Y[u]) / B.Y_BOUND:.3f} of the bound")
            assert abs(Y[u]) < B.Y_BOUND and frac >= 0.5
            img = np.frombuffer(b"".join(e.to_bytes(7, "little") * pre for e in elems), np.uint8)
            # (the vector in every slot of one chunk, so that the matrix-core kernel runs it)
            got = pos.left_multiply_unencoded_matrix_by_vectors(img, pre, np.array([left] * MFMA_MIN_VECS, np.uint64))
            want = sum(lw * e for lw, e in zip(left, elems)) * B.RINV % B.P
            assert [int(v) for v in got.reshape(-1)] == [want] * (pre * MFMA_MIN_VECS), (u, mirror)


def test_recombine63_at_the_bound(gpu):
    rng = random.Random(5)
    top = B.Y_BOUND - 1
    pd = [(B.P >> (8 * u)) & 0xff for u in range(8)]
    items = [pd, [-d for d in pd], [1] + [0] * 7, [-1] + [0] * 7, [0] * 8, [255, -1, 0, 0, 0, 0, 0, 0]]
    items += [[s * top] * 8 for s in (1, -1)]
    items += [[top if (k >> u) & 1 else -top for u in range(8)] for k in (0x55, 0xaa, 0x0f, 0xf0, 0x01, 0x80)]
    items += [[B.Y_BOUND] * 8, [-B.Y_BOUND] * 8]
    items += [[rng.randint(-B.Y_BOUND, B.Y_BOUND) for _ in range(8)] for _ in range(2000)]
    got = gpu.selftest_recombine63(np.array(items, np.int32))
    want = [B.recombine(y) for y in items]
    assert want[0] == 0 and want[1] == 0 and want[2] == B.RINV and want[3] == B.P - B.RINV   # sums of p, -p, 1, -1
    bad = [i for i, (g, w) in enumerate(zip(got.tolist(), want)) if g != w]
    assert not bad, f"{len(bad)} of {len(items)} differ; first: Y = {items[bad[0]]}, got {got[bad[0]]}, want {want[bad[0]]}"


def test_valu_only_child_gives_the_same_bytes(gpu, pos, tmp_path):
    """LCPC_NO_MFMA=1 is read once per process: a child recomputes the cases on the VALU kernel;
    every case also equals m calls of the single entry (pre = 24 packs first)."""
    import _pos_batch_child as child
    here = child.run_cases()
    out = tmp_path / "child.bin"
    r = subprocess.run([sys.executable, os.path.join(HERE, "_pos_batch_child.py"), str(out)],
                       env=dict(os.environ, LCPC_NO_MFMA="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == here
    singles = []
    for case in child.CHILD_CASES:
        data, lefts = child.inputs(case)
        assert pos.left_multiply_many_kernel(case[0], case[3]) == expected_kernel(case[0], case[3])
        singles += [pos.left_multiply_unencoded_matrix_by_vector(data.tobytes(), case[0], lv).tobytes() for lv in lefts]
    assert b"".join(singles) == here


def test_host_image_of_more_than_two_staging_blocks(gpu, pos):
    """One row more than two staging blocks (whole rows, an even number, near 8 MiB), m = 3, against
    three calls of the single entry."""
    pre = 64
    block_rows = ((8 << 20) // (7 * pre)) & ~1
    rows = 2 * block_rows + 1
    data = np.random.default_rng(8).integers(0, 256, 7 * pre * rows - 5, dtype=np.uint8)
    lefts = gpu.field_random(FT63, 3 * rows, 81).reshape(3, rows)
    got = pos.left_multiply_unencoded_matrix_by_vectors(data, pre, lefts)
    for t in range(3):
        assert np.array_equal(got[t], pos.left_multiply_unencoded_matrix_by_vector(data, pre, lefts[t]).reshape(-1)), t


# ---------------------------------------------------------------- protocol on a FileHandler
PRE, ENC, N_OPEN = 64, 128, 12


@pytest.fixture(scope="module")
def audit(gpu, pos, oracle, tmp_path_factory):
    """A stored file of about 100 KB with a ragged last row, five points and their vectors, then
    the columns drawn from a seed and opened -- in that order."""
    from lcpc_proof_of_storage_amd import pos_files
    tmp = tmp_path_factory.mktemp("batch_audit")
    data = np.random.default_rng(21).integers(0, 256, 7 * PRE * 223 + 19, dtype=np.uint8).tobytes()
    src = tmp / "file.bin"
    src.write_bytes(data)
    fh = pos_files.FileHandler.create_from_unencoded_file("01BATCHAUDIT00000000000000", str(src), PRE, ENC,
                                                          directory=str(tmp / "store"))
    points = oracle.ChaCha(seed_u64=4242, rounds=8).field_random(FT63, 5).reshape(-1)
    vectors = fh.batch_evaluation_vectors(points)
    idx = sorted(set(pos.get_column_indicies_from_random_seed(99, N_OPEN, ENC)))
    columns = fh.batch_evaluation_columns(idx)
    return dict(fh=fh, data=data, points=points, vectors=vectors, idx=idx, columns=columns, root=fh.get_commit_root())


def _verify(pos, a, **over):
    k = dict(points=a["points"], vectors=a["vectors"], idx=a["idx"], columns=a["columns"])
    k.update(over)
    return pos.client_verify_batch_evaluation(a["root"], len(a["data"]), PRE, ENC, k["points"], k["vectors"], k["idx"],
                                              k["columns"])


def test_batch_audit_returns_the_file_values(pos, oracle, audit):
    got = _verify(pos, audit)
    assert got.shape == (5, 1)
    xs = oracle.from_mont(FT63, audit["points"])
    assert oracle.from_mont(FT63, got.reshape(-1)) == [R.file_value(audit["data"], x) for x in xs]


def test_one_point_is_the_single_audit(gpu, pos, audit):
    fh, x = audit["fh"], audit["points"][:1]
    v = fh.batch_evaluation_vectors(x)
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(x, fh.rows_written, PRE)
    assert np.array_equal(v.reshape(-1), np.asarray(fh.left_multiply_unencoded_matrix_by_vector(left)).reshape(-1))
    result, opened = fh.polynomial_evaluation_response(x, audit["idx"])
    row = np.zeros((ENC, 1), np.uint64)
    row[:PRE, 0] = v[0]
    assert np.array_equal(gpu.LigeroEncoding.new_from_dims(FT63, PRE, ENC).encode(row), np.asarray(result).reshape(-1, 1))
    for a, b in zip(opened, audit["columns"]):
        assert np.array_equal(np.asarray(a.col), np.asarray(b.col)) and list(a.path) == list(b.path)
    single = pos._checked_file_evaluation(audit["root"], len(audit["data"]), PRE, ENC, x, audit["idx"], result, opened)
    assert np.array_equal(_verify(pos, audit, points=x, vectors=v).reshape(-1), single.reshape(-1))


def _single_kind(gpu, pos, audit, idx, columns):
    """the error the single audit raises for these columns"""
    x = audit["points"][:1]
    result, _ = audit["fh"].polynomial_evaluation_response(x, audit["idx"])
    with pytest.raises((gpu.VerifierError, ValueError)) as e:
        pos._checked_file_evaluation(audit["root"], len(audit["data"]), PRE, ENC, x, idx, result, columns)
    return type(e.value), getattr(e.value, "code", None)


def _tampered_columns(gpu, audit, which):
    cols = [gpu.LcColumn(np.array(c.col, copy=True), list(c.path)) for c in audit["columns"]]
    if which == "element":
        cols[3].col.reshape(-1)[17] ^= np.uint64(1)
    elif which == "path":
        p = bytearray(cols[5].path[1])
        p[0] ^= 1
        cols[5].path[1] = bytes(p)
    elif which == "length":
        cols[2] = gpu.LcColumn(np.array(cols[2].col, copy=True).reshape(-1)[:-1].reshape(-1, 1), cols[2].path)
    return cols


@pytest.mark.parametrize("which", ["element", "path", "length"])
def test_tampered_columns_are_rejected_as_in_the_single_audit(gpu, pos, audit, which):
    cols = _tampered_columns(gpu, audit, which)
    kind = _single_kind(gpu, pos, audit, audit["idx"], cols)
    with pytest.raises(gpu.VerifierError) as e:
        _verify(pos, audit, columns=cols)
    assert (type(e.value), e.value.code) == kind


def test_tampered_vectors_and_indices_are_rejected(gpu, pos, audit):
    v = audit["vectors"].copy()
    v[2, 40] ^= np.uint64(1)                       # one word of one vector
    with pytest.raises(gpu.VerifierError) as e:
        _verify(pos, audit, vectors=v)
    assert e.value.code == COLUMN_EVAL
    v = audit["vectors"].copy()
    v[4, 0] = np.uint64(B.P)                       # a word that is no field element
    with pytest.raises(gpu.VerifierError) as e:
        _verify(pos, audit, vectors=v)
    assert e.value.code == COLUMN_EVAL
    idx, cols = list(audit["idx"]), list(audit["columns"])
    idx[1], idx[2], cols[1], cols[2] = idx[2], idx[1], cols[2], cols[1]
    assert _single_kind(gpu, pos, audit, idx, cols)[0] is ValueError
    with pytest.raises(ValueError):
        _verify(pos, audit, idx=idx, columns=cols)


def test_a_vector_fitted_to_known_columns_fails_on_fresh_ones(gpu, pos, oracle, audit):
    """Why the order matters: a server that knows the columns adds to v_2 a polynomial that
    vanishes at their 12 evaluation points.  Against those columns the false vector passes (and a
    false value is returned); against columns drawn after the vectors were fixed it is rejected."""
    pts = oracle.from_mont(FT63, pos.rs_domain_points(FT63, ENC).reshape(-1))
    poly = [1]
    for c in audit["idx"]:                         # prod (X - pt_c), ascending coefficients
        poly = [((poly[i - 1] if i else 0) - pts[c] * (poly[i] if i < len(poly) else 0)) % B.P
                for i in range(len(poly) + 1)]
    assert len(poly) == len(audit["idx"]) + 1 <= PRE
    fitted = audit["vectors"].copy()
    for i, coeff in enumerate(poly):
        fitted[2, i] = np.uint64((int(fitted[2, i]) + coeff * B.R) % B.P)
    honest = _verify(pos, audit)
    cheated = _verify(pos, audit, vectors=fitted)
    assert not np.array_equal(cheated[2], honest[2]) and np.array_equal(np.delete(cheated, 2, 0), np.delete(honest, 2, 0))
    fresh = sorted(set(pos.get_column_indicies_from_random_seed(100, N_OPEN, ENC)))
    assert fresh != audit["idx"]
    fresh_columns = audit["fh"].batch_evaluation_columns(fresh)
    with pytest.raises(gpu.VerifierError) as e:
        _verify(pos, audit, vectors=fitted, idx=fresh, columns=fresh_columns)
    assert e.value.code == COLUMN_EVAL
    assert np.array_equal(_verify(pos, audit, idx=fresh, columns=fresh_columns), honest)
