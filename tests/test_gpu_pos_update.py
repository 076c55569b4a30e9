"""GPU: update audits end to end (pos.server_*_evaluation -> pos.client_verify_*_evaluation): every
corner of the row-range rule is accepted with the right value, every forged answer is rejected with
its kind, and the stored-file path answers as the commitment path does.  All comparisons are exact."""
import copy
import os
import shutil

import numpy as np
import pytest

import update_ref as R

pytestmark = pytest.mark.gpu
FT63 = 0
UNSUPPORTED = 34


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as P
    return P


@pytest.fixture(scope="module")
def point(oracle):
    x = oracle.ChaCha(seed_u64=1337, rounds=8).field_random(FT63, 1)
    return x, oracle.from_mont(FT63, x)[0]


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def corner_updates(pre):
    """(name, old_len, offset, length): the CPU grid's corners."""
    rb = 7 * pre
    ragged = 3 * rb + 5
    return [
        ("mid-coefficient start and end", ragged, 3, 9),
        ("across a row boundary", ragged, rb - 2, 5),
        ("the last byte", ragged, ragged - 1, 1),
        ("append inside the row", ragged, ragged, 4),
        ("append that fills the row", ragged, ragged, rb - 5),
        ("append that adds rows", ragged, ragged, 2 * rb + 1),
        ("append onto a row-aligned file", 2 * rb, 2 * rb, 10),
        ("overwrite that extends", ragged, ragged - 3, 10),
    ]


def _columns_for(oracle, nc, k, seed=5):
    return sorted(oracle.pos_column_indices(seed, k, nc))


def _check_server_against_oracle(pos, oracle, data, pre, nc, x, result, root):
    el = oracle.pos_bytes_to_field(data)
    oc = oracle.Commit(oracle.Encoding.ligero(FT63, pre, nc), el)
    assert root == oc.root()
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(x, oc.n_rows, pre)
    assert np.array_equal(np.asarray(result).reshape(-1), oracle.collapse(FT63, oc.comm, left.reshape(-1), oc.n_rows, nc))


def _run(pos, oracle, point, pre, nc, old_len, offset, length, n_open):
    x, xv = point
    old = _bytes(old_len, old_len + offset)
    data = _bytes(length, length + 17)
    new = R.apply_update(old, offset, data)
    cols = _columns_for(oracle, nc, n_open)
    resp = pos.server_update_evaluation(old, new, (pre, nc), x, cols, offset, length)
    _, _, old_lo, old_hi = R.update_rows(old_len, offset, length, pre)
    assert resp.original_bytes == old[old_lo:old_hi]
    _check_server_against_oracle(pos, oracle, old, pre, nc, x, resp.original_result_vector, resp.original_root)
    _check_server_against_oracle(pos, oracle, new, pre, nc, x, resp.new_result_vector, resp.new_root)
    got = pos.client_verify_update_evaluation(resp.original_root, resp.new_root, old_len, offset, data, pre, nc, x,
                                              cols, resp)
    assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(new, xv)
    return old, data, new, cols, resp


@pytest.mark.parametrize("pre,nc,n_open", [(4, 8, 3), (64, 128, 12)])
def test_update_corners_accept(pos, oracle, point, pre, nc, n_open):
    for name, old_len, offset, length in corner_updates(pre):
        _run(pos, oracle, point, pre, nc, old_len, offset, length, n_open)


def test_update_default_dims_three_rows(pos, oracle, point):
    """(16384, 32768): the one-pass encode, an edit across the boundary of rows 1 and 2 of 3."""
    pre, nc = 16384, 32768
    rb = 7 * pre
    _run(pos, oracle, point, pre, nc, 2 * rb + 100, 2 * rb - 2, 5, 6)


def test_wrappers_and_noop_edit(pos, oracle, point):
    x, xv = point
    pre, nc = 64, 128
    old = _bytes(3 * 7 * pre + 5, 1)
    cols = _columns_for(oracle, nc, 12)
    # an edit that writes the bytes already there: accepted, difference zero
    same = old[10:20]
    resp = pos.server_update_evaluation(old, old, (pre, nc), x, cols, 10, 10)
    got = pos.client_verify_edit_evaluation(resp.original_root, resp.new_root, len(old), 10, same, pre, nc, x, cols, resp)
    assert resp.original_root == resp.new_root
    assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(old, xv)
    tail = _bytes(33, 2)
    resp = pos.server_update_evaluation(old, old + tail, (pre, nc), x, cols)   # the range from the difference
    got = pos.client_verify_append_evaluation(resp.original_root, resp.new_root, len(old), tail, pre, nc, x, cols, resp)
    assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(old + tail, xv)
    with pytest.raises(ValueError):
        pos.client_verify_edit_evaluation(resp.original_root, resp.new_root, len(old), len(old) - 1, b"ab", pre, nc, x,
                                          cols, resp)


def _rejected(pos, kind, *args):
    with pytest.raises(pos.VerifierError) as e:
        pos.client_verify_update_evaluation(*args)
    assert e.value.kind == kind, e.value


def test_update_forgeries_rejected(pos, oracle, point):
    x, _ = point
    pre, nc = 64, 128
    rb = 7 * pre
    old_len, offset, length = 3 * rb + 5, rb - 2, 5
    old, data, new, cols, resp = _run(pos, oracle, point, pre, nc, old_len, offset, length, 12)
    roots = (resp.original_root, resp.new_root)
    args = (old_len, offset, data, pre, nc, x)

    # a flipped byte in original_bytes
    bad = copy.deepcopy(resp)
    bad.original_bytes = bytes([bad.original_bytes[0] ^ 1]) + bad.original_bytes[1:]
    _rejected(pos, "RowsMismatch", *roots, *args, cols, bad)
    bad.original_bytes = resp.original_bytes[:-1]
    _rejected(pos, "RowsMismatch", *roots, *args, cols, bad)

    # a new file that differs from the client's data inside the range.  Every codeword position of a
    # row depends on every element of it, so any opened column sees the change; with no column
    # opened only the difference of the evaluations does.
    forged = bytearray(new)
    forged[offset + 1] ^= 0x40
    seen = pos.server_update_evaluation(old, bytes(forged), (pre, nc), x, cols, offset, length)
    _rejected(pos, "RowsMismatch", seen.original_root, seen.new_root, *args, cols, seen)
    unseen = pos.server_update_evaluation(old, bytes(forged), (pre, nc), x, [], offset, length)
    _rejected(pos, "UpdateMismatch", unseen.original_root, unseen.new_root, *args, [], unseen)

    # a new file that also changes an untouched row (row 3), the result vector recomputed honestly
    forged = bytearray(new)
    forged[3 * rb + 1] ^= 1
    seen = pos.server_update_evaluation(old, bytes(forged), (pre, nc), x, cols, offset, length)
    _rejected(pos, "RowsMismatch", seen.original_root, seen.new_root, *args, cols, seen)
    unseen = pos.server_update_evaluation(old, bytes(forged), (pre, nc), x, [], offset, length)
    _rejected(pos, "UpdateMismatch", unseen.original_root, unseen.new_root, *args, [], unseen)

    # a tampered result entry
    bad = copy.deepcopy(resp)
    bad.new_result_vector[cols[2], 0] ^= np.uint64(1)
    _rejected(pos, "ColumnEval", *roots, *args, cols, bad)
    # a wrong path digest
    bad = copy.deepcopy(resp)
    p0 = bad.new_columns[1].path[0]
    bad.new_columns[1].path[0] = bytes([p0[0] ^ 1]) + p0[1:]
    _rejected(pos, "ColumnEval", *roots, *args, cols, bad)
    # a stale new_root
    _rejected(pos, "ColumnEval", resp.original_root, resp.original_root, *args, cols, resp)
    # the honest answer still passes
    pos.client_verify_update_evaluation(*roots, *args, cols, resp)


@pytest.mark.parametrize("new_dims", [(32, 64), (128, 256)])
def test_reshape(pos, oracle, point, new_dims):
    x, xv = point
    old_dims = (64, 128)
    data = _bytes(7 * 64 * 9 + 3, 7)
    cols_old = _columns_for(oracle, old_dims[1], 10)
    cols_new = _columns_for(oracle, new_dims[1], 10, seed=6)
    resp = pos.server_reshape_evaluation(data, old_dims, new_dims, x, cols_old, cols_new)
    _check_server_against_oracle(pos, oracle, data, *old_dims, x, resp.original_result_vector, resp.original_root)
    _check_server_against_oracle(pos, oracle, data, *new_dims, x, resp.new_result_vector, resp.new_root)
    want = R.file_value(data, xv)
    assert oracle.from_mont(FT63, np.asarray(resp.expected_result).reshape(-1))[0] == want
    got = pos.client_verify_reshape_evaluation(resp.original_root, resp.new_root, len(data), old_dims, new_dims, x,
                                               cols_old, cols_new, resp)
    assert oracle.from_mont(FT63, got.reshape(-1))[0] == want
    # a server that reshapes a different file
    other = bytearray(data)
    other[100] ^= 1
    forged = pos.server_reshape_evaluation(bytes(other), old_dims, new_dims, x, cols_old, cols_new)
    with pytest.raises(pos.VerifierError):
        pos.client_verify_reshape_evaluation(resp.original_root, forged.new_root, len(data), old_dims, new_dims, x,
                                             cols_old, cols_new, forged)
    bad = copy.deepcopy(resp)
    bad.expected_result = np.asarray(bad.expected_result).copy()
    bad.expected_result.reshape(-1)[0] ^= np.uint64(1)
    with pytest.raises(pos.VerifierError) as e:
        pos.client_verify_reshape_evaluation(resp.original_root, resp.new_root, len(data), old_dims, new_dims, x,
                                             cols_old, cols_new, bad)
    assert e.value.kind == "ReshapeMismatch"


def test_other_digest_is_unsupported(gpu, pos, point):
    x, _ = point
    enc = gpu.LigeroEncoding.new_from_dims(FT63, 64, 128)
    other = gpu.LigeroEncoding.new_from_dims(FT63, 64, 128)
    other.set_digest(1)
    with pos._DeviceImage(_bytes(7 * 64 * 3, 3)) as d:
        with pytest.raises(gpu.LcpcError) as e:
            pos._update_evaluation(enc, d.ptr, d.n, other, d.ptr, d.n, x, [1], [1], False)
    assert e.value.code == UNSUPPORTED


# ---------------------------------------------------------------- stored files
@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def _handler(PF, tmp_path, name, data, pre, nc):
    src = tmp_path / f"{name}.bin"
    src.write_bytes(data)
    return PF.FileHandler.create_from_unencoded_file(name, str(src), pre, nc, directory=str(tmp_path / name))


@pytest.mark.parametrize("n_bytes", [1000, 7 * 64 * 40 - 11])
def test_stored_file_response_equals_the_commitment_path(gpu, pos, PF, oracle, point, tmp_path, n_bytes):
    x, _ = point
    pre, nc = 64, 128
    data = _bytes(n_bytes, n_bytes)
    fh = _handler(PF, tmp_path, "01RESPONSE0000000000000000", data, pre, nc)
    cols = _columns_for(oracle, nc, 12)
    result, opened = fh.polynomial_evaluation_response(x, cols)
    enc = gpu.LigeroEncoding.new_from_dims(FT63, pre, nc)
    comm = gpu.LcCommit.commit_pos_bytes(data, enc)
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(x, comm.get_n_rows(), pre)
    assert fh.get_commit_root() == comm.get_root()
    assert np.array_equal(np.asarray(result).reshape(-1), pos.verifiable_polynomial_evaluation(comm, left).reshape(-1))
    for a, b in zip(opened, comm.open_columns(cols)):
        assert np.array_equal(np.asarray(a.col).reshape(-1), b.col.reshape(-1)) and list(a.path) == list(b.path)


def test_stored_file_edit_and_append_verify(pos, PF, oracle, point, tmp_path):
    """edit_bytes / append_bytes on a copy of the stored files; the two handlers' answers, put
    together as the server's message, verify against the two handlers' roots."""
    x, xv = point
    pre, nc = 64, 128
    ulid = "01UPDATE000000000000000000"
    data = _bytes(7 * pre * 5 + 20, 31)
    before = _handler(PF, tmp_path, ulid, data, pre, nc)
    cols = _columns_for(oracle, nc, 12)
    for step, (offset, patch) in enumerate([(7 * pre - 3, _bytes(11, 32)), (len(data), _bytes(7 * pre + 9, 33))]):
        old = open(before.get_raw_file_handle(), "rb").read()
        copy_dir = tmp_path / f"copy{step}"
        shutil.copytree(os.path.dirname(before.get_raw_file_handle()), copy_dir)
        after = PF.FileHandler.new_attach_to_existing_ulid(str(copy_dir), ulid)
        if offset == len(old):
            after.append_bytes(patch)
        else:
            after.edit_bytes(offset, patch)
        _, _, old_lo, old_hi = pos.update_rows(len(old), offset, len(patch), pre)
        r_old, c_old = before.polynomial_evaluation_response(x, cols)
        r_new, c_new = after.polynomial_evaluation_response(x, cols)
        resp = pos.UpdateEvaluation(r_old, c_old, r_new, c_new, before.get_unencoded_bytes(old_lo, old_hi))
        got = pos.client_verify_update_evaluation(before.get_commit_root(), after.get_commit_root(), len(old), offset,
                                                  patch, pre, nc, x, cols, resp)
        assert oracle.from_mont(FT63, got.reshape(-1))[0] == R.file_value(R.apply_update(old, offset, patch), xv)
        before = after
