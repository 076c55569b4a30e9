"""Child process of test_gpu_pool_poison.py: every kind of device and staging buffer the library takes
from its pools, exercised on two data sets of identical shapes.

A and B have the same shapes (so every pool block has the same size and comes back into the same role)
but different bytes and OPPOSITE verdict patterns: the jobs, rows and columns that are damaged,
non-canonical, forged or refused in A are clean in B and the other way round.  `--order ab` runs all of A
and then all of B, `--order b` B alone; either prints one JSON line {case: sha256 of everything the case
returned for B}.  A word that B's calls forget to write still holds A's value (or, under
LCPC_POOL_POISON, the poison) and changes the digest.  Where a call has a known truth it is asserted
here: decoded rows are the codewords, located positions the injected ones, a repaired file the undamaged
one, verdicts the injected pattern.

Before each case its name goes to stderr (flushed): a run that dies names its case in the log.
`--parts FILE` also writes the parts the parent compares with the oracle (an .npz); `--probe` runs the
allocator's own selftest instead of the cases."""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import lcpc_proof_of_storage_amd as L  # noqa: E402
from lcpc_proof_of_storage_amd import pos, pos_files as PF  # noqa: E402

FT63, FT127, FT191 = 0, 1, 2
P63 = pos.FT63_MODULUS
FF = np.uint64(0xFFFFFFFFFFFFFFFF)
UNRECOVERABLE = 36
LIGERO_LEN = (1 << 14) + 77
FUSED_DIMS = (1 << 14, 1 << 15)       # the smallest Ft127 RsEncoding whose pass B also hashes the leaves ...
FUSED_LEN = 3 * (1 << 14)             # ... for device-resident whole rows
SDIG_LEN = 3000
BATCH_LG = 10
DIGEST_LEN = 1 << 12
POS_BYTES = 7 * 64 * 9 + 5
POS_DIMS = (64, 128)
HASH_SHAPES = [(FT63, 124, 16), (FT63, 125, 16), (FT63, 1021, 16), (FT191, 100, 8)]
DECODER_SHAPES = [(16, 32), (512, 1024)]
DECODER_ROWS = 130
FILE_DIMS = [(24, 32), (64, 128)]
FLEET_DIMS = [(1, 2), (8, 16), (24, 32), (15, 16), (100, 256), (512, 1024)]
FLEET_ROWS = [0, 1, 7, 8, 9, 17, 125]
FLEET_N = 36
# the widths the grouped u^T M kernel takes (every other pre is the single call inside the grouped one, by
# the plan): the audit fleet keeps the dims' encs and row counts at these
AUDIT_DIMS = [(32, 64), (8, 16), (16, 32), (128, 256), (64, 256), (512, 1024)]

CASES = ([f"ligero_f{f}" for f in range(5)] + ["ligero_device_f1", "ligero_fused_f1", "sdig_f0", "sdig_f1",
         "batch_f0", "batch_f1", "digest_sha256", "digest_sha3_256", "pos_bytes", "hash_columns", "merkle_tree"]
         + [f"decoders_f{f}_{n}_{m}" for f in (FT63, FT191) for n, m in DECODER_SHAPES]
         + [f"files_{p}_{e}_{'cache' if c else 'plain'}" for p, e in FILE_DIMS for c in (False, True)]
         + ["group_ingest", "group_scrub", "group_repair", "group_audit", "group_verify", "sharded_n1"])


def seed_of(which: str, k: int = 0) -> int:
    return {"A": 100_000, "B": 200_000}[which] + k


# ---------------------------------------------------------------- what a case returns
class Result:
    """everything a case returned, in call order: the digest, and the parts kept for the parent"""

    def __init__(self, name, keep):
        self.name, self.h, self.keep, self.parts = name, hashlib.sha256(), keep, {}

    def add(self, key, value, part=False):
        if isinstance(value, (bytes, bytearray)):
            b = bytes(value)
        elif isinstance(value, np.ndarray):
            b = str(value.dtype).encode() + repr(value.shape).encode() + np.ascontiguousarray(value).tobytes()
        else:
            b = json.dumps(value, sort_keys=True).encode()
        self.h.update(key.encode() + b"\0" + len(b).to_bytes(8, "little"))
        self.h.update(b)
        if part and self.keep:
            self.parts[f"{self.name}/{key}"] = np.frombuffer(b, np.uint8) if isinstance(value, (bytes, bytearray)) \
                else np.asarray(value)


def tr(root):
    t = L.Transcript(b"pool poison")
    t.append_message(b"polycommit", root)
    return t


def verdict(fn):
    """what a verifier said: ('ok', value) or ('refused', kind)"""
    try:
        return "ok", fn()
    except L.VerifierError as e:
        return "refused", e.kind


# ---------------------------------------------------------------- inputs (the parent rebuilds them)
def ligero_coeffs(which, field):
    return L.field_random(field, LIGERO_LEN, seed_of(which, 11 + field))


def fused_coeffs(which):
    return L.field_random(FT127, FUSED_LEN, seed_of(which, 17))


def sdig_coeffs(which, field):
    return L.field_random(field, SDIG_LEN, seed_of(which, 31 + field))


def batch_coeffs(which, field):
    return L.field_random(field, 1 << BATCH_LG, seed_of(which, 41 + field))


def batch_outers(which, field, n_rows):
    return [L.field_random(field, n_rows, seed_of(which, 50 + 3 * field + j)) for j in range(3)]


def digest_coeffs(which):
    return L.field_random(FT127, DIGEST_LEN, seed_of(which, 61))


def hash_matrix(which, k):
    field, rows, cols = HASH_SHAPES[k]
    return L.field_random(field, rows * cols, seed_of(which, 70 + k))


def merkle_leaves(which):
    return np.random.default_rng(seed_of(which, 80)).integers(0, 256, 1024 * 32, dtype=np.uint8).tobytes()


def file_bytes(which, k, n):
    return np.random.default_rng(seed_of(which, 1000 + k)).integers(0, 256, n, dtype=np.uint8)


def fleet(which):
    """the 36 files of the grouped entries: (bytes, pre, enc, rows), the last row 3 bytes short"""
    out = []
    for j in range(FLEET_N):
        pre, enc = FLEET_DIMS[j % len(FLEET_DIMS)]
        rows = FLEET_ROWS[j % len(FLEET_ROWS)]
        out.append((file_bytes(which, j, max(rows * 7 * pre - 3, 0)), pre, enc, rows))
    return out


def is_bad(which, j):
    """A: every third job; B: their neighbours.  No job is bad in both."""
    return j % 3 == (0 if which == "A" else 1)


# ---------------------------------------------------------------- commit / prove / verify
def prove_verify(res, enc, coeffs, field, seed, c=None):
    c = L.LcCommit.commit(coeffs, enc) if c is None else c
    root, n_rows = c.get_root(), c.get_n_rows()
    outer = L.field_random(field, n_rows, seed + 1)
    inner = L.field_random(field, enc.n_per_row, seed + 2)
    pf = c.prove(outer, enc, tr(root))
    ev = pf.verify(root, outer, inner, enc, tr(root))
    res.add("root", root, part=True)
    res.add("comm", c.comm)
    res.add("proof", pf.to_bincode())
    res.add("p_eval", np.asarray(pf.p_eval), part=True)
    res.add("p_random", np.stack([np.asarray(v) for v in pf.p_random_vec]), part=True)
    res.add("ev", np.ascontiguousarray(ev), part=True)
    # a forged root is refused, whatever the verifier's scratch held
    bad = bytes([root[0] ^ 1]) + root[1:]
    v = verdict(lambda: pf.verify(bad, outer, inner, enc, tr(bad)))
    assert v[0] == "refused", v
    res.add("forged_root", v[1])
    return c


def case_ligero(res, which, field):
    coeffs = ligero_coeffs(which, field)
    prove_verify(res, L.LigeroEncoding.new(field, LIGERO_LEN), coeffs, field, seed_of(which, 20 + field))


def case_ligero_device(res, which, hm):
    """the same length from device-resident coefficients (lcpc_commit_new_device; the cases above commit
    host-resident ones, lcpc_commit_new)"""
    coeffs = ligero_coeffs(which, FT127)
    enc = L.LigeroEncoding.new(FT127, LIGERO_LEN)
    d = hm.to_device(coeffs)
    try:
        c = L.LcCommit.commit_device(d, LIGERO_LEN, enc)
        root = c.get_root()
        assert root == L.LcCommit.commit(coeffs, enc).get_root()
        res.add("root", root, part=True)
        res.add("comm", c.comm)
        res.add("coeffs", c.coeffs)
    finally:
        hm.free(d)


def case_ligero_fused(res, which, hm):
    enc = L.RsEncoding.new(FT127, FUSED_DIMS[0], FUSED_DIMS[1], 24, 2)
    # (a build without the kernel says so, as tests/test_gpu_ntt_leaf_fuse.py has it)
    assert enc.leaf_fuse == (os.environ.get("LCPC_NTT_LEAF_FUSE_BUILD", "1") != "0"), "the fused leaf pass is what this case is for"
    coeffs = fused_coeffs(which)
    d = hm.to_device(coeffs)
    try:
        c = L.LcCommit.commit_device(d, FUSED_LEN, enc)
        prove_verify(res, enc, coeffs, FT127, seed_of(which, 27), c)
    finally:
        hm.free(d)


def case_sdig(res, which, field):
    enc = L.SdigEncoding.new(field, SDIG_LEN, 5, 3)
    assert enc.n_cols & (enc.n_cols - 1), "a codeword that is no power of two"
    prove_verify(res, enc, sdig_coeffs(which, field), field, seed_of(which, 35 + field))


def case_batch(res, which, field):
    """3 points (Ft127: the matrix-core many-tensor kernel, Ft63: the VALU one); the forged verify sits
    in A for Ft63 and in B for Ft127"""
    enc = L.LigeroEncoding.new(field, 1 << BATCH_LG)
    coeffs = batch_coeffs(which, field)
    c = L.LcCommit.commit(coeffs, enc)
    root, n_rows = c.get_root(), c.get_n_rows()
    outers = batch_outers(which, field, n_rows)
    inners = [L.field_random(field, enc.n_per_row, seed_of(which, 56 + j)) for j in range(3)]
    pf = c.prove_batch(outers, enc, tr(root))
    evs = pf.verify(root, outers, inners, enc, tr(root))
    res.add("root", root, part=True)
    res.add("proof", pf.to_bytes())
    res.add("p_evals", np.stack([np.asarray(v) for v in pf.p_eval_vec]), part=True)
    res.add("evs", np.stack(evs))
    if (which == "A") == (field == FT63):
        cols = pf.columns
        col = np.array(cols[1].col, np.uint64).copy()
        col.reshape(-1)[0] ^= np.uint64(1)
        cols[1] = L.LcColumn(col, cols[1].path)
        forged = L.LcBatchEvalProof.from_parts(field, pf.n_cols, pf.p_eval_vec, pf.p_random_vec, cols)
        v = verdict(lambda: forged.verify(root, outers, inners, enc, tr(root)))
        assert v[0] == "refused", v
        res.add("forged", v[1])
    else:
        again = pf.verify(root, outers, inners, enc, tr(root))
        assert all(np.array_equal(a, b) for a, b in zip(again, evs))
        res.add("again", np.stack(again))


def case_digest(res, which, digest):
    enc = L.LigeroEncoding.new(FT127, DIGEST_LEN)
    enc.set_digest(digest)
    prove_verify(res, enc, digest_coeffs(which), FT127, seed_of(which, 64 + digest))


# ---------------------------------------------------------------- a file image in memory
def case_pos_bytes(res, which):
    pre, enc = POS_DIMS
    data = file_bytes(which, 900, POS_BYTES)
    code = L.RsEncoding.new(FT63, pre, enc, 16, 2)
    c = L.LcCommit.commit_pos_bytes(data, code)
    root, rows = c.get_root(), c.get_n_rows()
    assert rows == 10
    res.add("root", root)
    res.add("comm", c.comm)
    res.add("coeffs", c.coeffs)
    # the evaluation request and the client's check; A's response is forged, B's honest
    point = L.field_random(FT63, 1, seed_of(which, 901))
    left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(point, rows, pre)
    result = pos.verifiable_polynomial_evaluation(c, left)
    cols = [3, 17, 64, 127]
    opened = c.open_columns(cols)
    res.add("result", np.asarray(result))
    if which == "A":
        result = np.array(result, np.uint64).copy()
        result.reshape(-1)[5] ^= np.uint64(4)
    v = verdict(lambda: pos.client_verify_evaluation(root, POS_BYTES, pre, enc, point, cols, result, opened))
    assert v[0] == ("refused" if which == "A" else "ok"), v
    res.add("client", v[1] if v[0] == "refused" else np.asarray(v[1]))
    value = pos.evaluate_bytes_polynomial_at_point(data.tobytes(), point)
    if which == "B":
        assert np.array_equal(np.asarray(v[1]).reshape(-1), value.reshape(-1))
    res.add("eval_poly", value)
    for m in (3, 16):   # the VALU and the matrix-core contraction
        lefts = np.random.default_rng(seed_of(which, 910 + m)).integers(0, P63, (m, rows), dtype=np.uint64)
        many = pos.left_multiply_unencoded_matrix_by_vectors(data, pre, lefts)
        one = pos.left_multiply_unencoded_matrix_by_vector(data.tobytes(), pre, lefts[m - 1])
        assert np.array_equal(many[m - 1], np.asarray(one).reshape(-1))
        res.add(f"left_{m}", many)


def case_hash_columns(res, which):
    for k, (field, rows, cols) in enumerate(HASH_SHAPES):
        res.add(f"hash_{k}", L.hash_columns(field, hash_matrix(which, k), rows, cols), part=True)


def case_merkle_tree(res, which):
    res.add("tree", L.merkle_tree(merkle_leaves(which)), part=True)


# ---------------------------------------------------------------- row decoders
def case_decoders(res, which, field, npr, length):
    """130 rows, dirty and clean alternating (A's dirty rows are B's clean ones), 0 / 1 / N/2 wrong
    positions and one erasure set; A ends with an over-radius batch of the same shape (refused), which is
    what B's decodable batch finds in the pool"""
    nl = L.limbs(field)
    code = L.LigeroEncoding.new_from_dims(field, npr, length)
    msgs = L.field_random(field, DECODER_ROWS * npr, seed_of(which, 300 + field + length)).reshape(DECODER_ROWS, npr, nl)
    cw = np.zeros((DECODER_ROWS, length, nl), np.uint64)
    cw[:, :npr] = msgs
    cw = code.encode_rows(cw).copy()
    rng = np.random.default_rng(seed_of(which, 310 + field + length))
    n_erased = (length - npr) // 4
    erased = sorted(int(c) for c in rng.permutation(length)[:n_erased])
    avail = np.array([c for c in range(length) if c not in erased])
    N = length - npr - n_erased
    junk = L.field_random(field, DECODER_ROWS * (N // 2 + 1), seed_of(which, 320 + field + length)).reshape(-1, nl)
    parity = 0 if which == "A" else 1

    def damaged(counts):
        rows, where, k = cw.copy(), [], 0
        for r, t in enumerate(counts):
            at = sorted(int(c) for c in rng.choice(avail, size=t, replace=False)) if t else []
            for c in at:
                assert not np.array_equal(junk[k], cw[r, c])
                rows[r, c] = junk[k]
                k += 1
            where.append(at)
        rows[:, erased] = FF
        return rows, where

    counts = [(1, N // 2)[(r // 2) % 2] if r % 2 == parity else 0 for r in range(DECODER_ROWS)]
    rows, where = damaged(counts)
    keep = rows.copy()
    status, n_err, mask, col_any = pos.locate_errors_rows(field, rows, npr, erased)
    assert np.array_equal(rows, keep)
    want_any = np.zeros(length, np.uint8)
    for r, at in enumerate(where):
        assert (int(status[r]), int(n_err[r])) == ((1, len(at)) if at else (0, 0)), (r, at)
        assert [int(c) for c in np.flatnonzero(mask[r])] == at, r
        want_any[at] = 1
    assert np.array_equal(col_any, want_any)
    for k, v in (("status", status), ("n_err", n_err), ("mask", mask), ("col_any", col_any)):
        res.add(k, v)
    # erasures alone (the clean rows), and the consistency check of a dirty batch
    clean = [r for r in range(DECODER_ROWS) if not where[r]]
    filled = pos.erasure_decode_rows(field, rows[clean], npr, erased)
    assert np.array_equal(filled, cw[clean])
    res.add("erasure", filled)
    try:
        pos.erasure_decode_rows(field, rows, npr, erased)
        raise AssertionError("a dirty batch passed the erasure decoder's check")
    except L.LcpcError as e:
        assert e.code == UNRECOVERABLE, e
    if which == "A":   # over the radius: refused, nothing written
        over, _ = damaged([N // 2 + 1 if r % 2 == parity else 0 for r in range(DECODER_ROWS)])
        keep = over.copy()
        try:
            pos.decode_rows(field, over, npr, erased)
            raise AssertionError("an over-radius batch was decoded")
        except L.LcpcError as e:
            assert e.code == UNRECOVERABLE, e
        assert np.array_equal(over, keep)
        res.add("over_radius", "refused")
    fixed = pos.decode_rows(field, rows, npr, erased)
    assert np.array_equal(fixed, cw)
    res.add("decoded", fixed)


# ---------------------------------------------------------------- stored files
def _read(p):
    with open(p, "rb") as f:
        return f.read()


def _poke(path, offset, data):
    with open(path, "r+b") as f:
        f.seek(offset)
        f.write(data)


def _snapshot(fh):
    return {k: _read(p) for k, p in (("raw", fh.get_raw_file_handle()), ("enc", fh.get_encoded_file_handle()),
                                     ("tree", fh.get_merkle_file_handle()))}


def _written(image, enc, cap, rows):
    return np.frombuffer(image, np.uint8).reshape(enc, cap * 8)[:, :rows * 8]


def _report(rep):
    return [rep.bad_columns, rep.noncanonical_columns, rep.tree_consistent, rep.root_ok, rep.raw_ok, rep.repaired_from,
            rep.located_columns, rep.unlocatable_rows]


def case_files(res, which, pre, enc, cache, tmp):
    ulid = "01POOLPOISON00000000000000"
    d = os.path.join(tmp, f"{which}_{pre}_{enc}_{int(cache)}")
    os.makedirs(d)
    rb = 7 * pre
    data = file_bytes(which, 500 + pre, 126 * rb - 3).tobytes()
    src = os.path.join(d, "in.bin")
    with open(src, "wb") as f:
        f.write(data)
    fh = PF.FileHandler.create_from_unencoded_file(ulid, src, pre, enc, directory=os.path.join(d, "store"),
                                                   chunk_cache=cache)
    assert fh.rows_written == 126
    res.add("root_126", fh.get_commit_root())
    # an edit in the middle, then appends across the 252 / 253-row seam of the leaves' chunks
    patch = file_bytes(which, 510 + pre, 3 * rb + 11).tobytes()
    old, tree = fh.edit_bytes(40 * rb + 5, patch)
    assert old == data[40 * rb + 5:40 * rb + 5 + len(patch)]
    old_data = data
    data = data[:40 * rb + 5] + patch + data[40 * rb + 5 + len(patch):]
    res.add("root_edit", tree.root())
    # the update audit of that edit: honest in B, a forged new root in A
    point = L.field_random(FT63, 1, seed_of(which, 520 + pre))
    cols = [1, enc // 2, enc - 1]
    old_root = L.LcCommit.commit_pos_bytes(old_data, L.LigeroEncoding.new_from_dims(FT63, pre, enc)).get_root()
    resp = pos.server_update_evaluation(old_data, data, (pre, enc), point, cols, 40 * rb + 5, len(patch))
    new_root = tree.root() if which == "B" else bytes([tree.root()[0] ^ 1]) + tree.root()[1:]
    v = verdict(lambda: pos.client_verify_edit_evaluation(old_root, new_root, len(old_data), 40 * rb + 5, patch, pre, enc,
                                                          point, cols, resp))
    assert v[0] == ("ok" if which == "B" else "refused"), v
    res.add("update_audit", v[1] if v[0] == "refused" else np.asarray(v[1]))
    for k, n in enumerate((126 * rb + 3, rb, 5)):     # to 252 rows exactly, to 253, and a few bytes more
        more = file_bytes(which, 530 + pre + k, n).tobytes()
        tree = fh.append_bytes(more)
        data += more
        res.add(f"root_append_{k}", tree.root())
    assert fh.rows_written == 254 and _read(fh.get_raw_file_handle()) == data
    fh.verify_all_files_agree()
    root = fh.get_commit_root()
    # a checkable read across the seam
    a, b = 251 * rb - 9, 253 * rb + 2
    rows_msg = fh.read_rows_response(a, b)
    rcols = [0, 5, enc - 2]
    opening = fh.read_opening_response(a, b, rcols)
    got = pos.client_verify_read(root, len(data), pre, enc, a, b, rows_msg, rcols, opening, seed=7)
    assert got == data[a:b]
    res.add("read_segments", opening.segments)
    res.add("read_covers", opening.covers)
    # the audit answered from the stored files, checked by the client
    result, opened = fh.polynomial_evaluation_response(point, cols)
    value = pos.client_verify_evaluation(root, len(data), pre, enc, point, cols, result, opened)
    assert np.array_equal(value.reshape(-1), pos.evaluate_bytes_polynomial_at_point(data, point).reshape(-1))
    res.add("audit", np.asarray(result))
    res.add("audit_value", np.asarray(value))
    # damage: two columns and one non-canonical element; A's columns are not B's
    sound = _snapshot(fh)
    rows, cap = fh.rows_written, fh.row_capacity
    bad = [1, 5] if which == "A" else [2, 7]
    nonc = 9 if which == "A" else 12
    rng = np.random.default_rng(seed_of(which, 540 + pre))
    for c in bad:
        _poke(fh.get_encoded_file_handle(), c * cap * 8, rng.integers(0, 256, rows * 8, dtype=np.uint8).tobytes())
    _poke(fh.get_encoded_file_handle(), (nonc * cap + 100) * 8, b"\xff" * 8)
    want = sorted(bad + [nonc])
    rep = fh.scrub(expected_root=root)
    assert rep.bad_columns == want and nonc in rep.noncanonical_columns and rep.tree_consistent and rep.raw_ok, rep
    assert rep.root_ok is True and not rep.clean
    res.add("scrub", _report(rep))
    rep = fh.scrub(locate=True)
    assert rep.bad_columns == want and sorted(rep.located_columns) == want and rep.unlocatable_rows == 0, rep
    res.add("scrub_locate", _report(rep))
    rep = fh.repair(expected_root=root)
    assert rep.bad_columns == want and rep.repaired_from == "columns", rep
    res.add("repair", _report(rep))
    now = _snapshot(fh)
    assert np.array_equal(_written(now["enc"], enc, cap, rows), _written(sound["enc"], enc, cap, rows))
    assert now["tree"] == sound["tree"] and now["raw"] == sound["raw"]
    again = fh.scrub(expected_root=root)
    assert again.clean and again.bad_columns == [], again
    res.add("scrub_after", _report(again))
    fh.delete_all_files()


# ---------------------------------------------------------------- grouped entries
_fleet_made = {}


def stored_fleet(which):
    """the fleet as stored files: per file (image bytes, tree, pre, enc, rows, cap), capacity 2 rows + 3
    prefilled with 0xA5; made by one lcpc_pos_encode_file per file, so the grouped calls meet them fresh"""
    import ctypes as C
    from lcpc_proof_of_storage_amd import _native as N
    if which not in _fleet_made:
        lib, out = N.load(), []
        u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None  # noqa: E731
        for data, pre, enc, rows in fleet(which):
            cap = 2 * rows + 3
            img = np.full(enc * cap * 8, 0xA5, np.uint8)
            tree = np.zeros((2 * enc - 1, 32), np.uint8)
            got = C.c_size_t()
            assert lib.lcpc_pos_encode_file(u8(data), data.size, pre, enc, cap, u8(img), u8(tree), C.byref(got)) == 0
            assert got.value == rows
            out.append((img, tree, pre, enc, rows, cap))
        _fleet_made[which] = out
    return _fleet_made[which]


def no_single(tiles, groups):
    assert groups == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any(), "a job left the grouped path"


def case_group_ingest(res, which):
    files = fleet(which)
    datas, pres, encs = [f[0] for f in files], [f[1] for f in files], [f[2] for f in files]
    no_single(*pos.ingest_plan([d.size for d in datas], pres, encs))
    caps = [2 * f[3] + 3 for f in files]
    imgs = [np.full(e * c * 8, 0xA5, np.uint8) for e, c in zip(encs, caps)]
    out = pos.encode_files_grouped_into(datas, pres, encs, imgs, caps, True, True, True)
    for j, (o, f) in enumerate(zip(out, files)):
        assert o["rows_written"] == f[3] and o["root"] == o["tree"][-1].tobytes(), j
        res.add(f"img_{j}", imgs[j], part=True)
        res.add(f"tree_{j}", o["tree"], part=True)
        res.add(f"cvs_{j}", o["cvs"])


def case_group_scrub(res, which):
    """a bad job has one flipped bit, one all-ones word or one forged stored leaf, by turns"""
    files = [(img.copy(), tree.copy(), pre, enc, rows, cap) for img, tree, pre, enc, rows, cap in stored_fleet(which)]
    no_single(*pos.scrub_plan([f[4] for f in files], [f[2] for f in files], [f[3] for f in files]))
    roots = [f[1][-1].tobytes() for f in files]
    expect = []
    for j, (img, tree, pre, enc, rows, cap) in enumerate(files):
        if not is_bad(which, j):
            expect.append(None)
            continue
        kind = (j // 3) % 3 if rows else 2
        c = (5 * j + 1) % enc
        el = img.view("<u8").reshape(enc, cap)
        if kind == 0:
            el[c, (3 * j) % rows] ^= np.uint64(1 << (j % 32))
        elif kind == 1:
            el[c, (3 * j) % rows] = FF
        else:
            tree[c, 7] ^= 0x10
        expect.append((kind, c))
    out = pos.scrub_files_grouped([f[0] for f in files], [f[2] for f in files], [f[3] for f in files],
                                  [f[4] for f in files], [f[5] for f in files], [f[1] for f in files], roots,
                                  want_digests=True)
    for j, (r, f, e) in enumerate(zip(out, files, expect)):
        if e is None:
            assert not r["status"].any() and r["n_bad"] == 0 and r["n_dirty_rows"] == 0, j
            assert r["tree_consistent"] is True and r["root_ok"] is True, j
            assert np.array_equal(r["digests"], f[1][:f[3]]), j
        else:
            kind, c = e
            assert list(np.flatnonzero(r["status"])) == [c] and r["n_bad"] == 1, (j, e, r["status"])
            assert r["status"][c] == (2 if kind == 1 else 1), (j, e)
            assert r["n_dirty_rows"] == (None if kind == 1 else 1 if kind == 0 else 0), (j, e, r["n_dirty_rows"])
            assert r["tree_consistent"] is (kind != 2) and r["root_ok"] is True, (j, e)
        res.add(f"status_{j}", r["status"])
        res.add(f"digests_{j}", r["digests"])
        res.add(f"flags_{j}", [r["n_bad"], r["n_dirty_rows"], r["tree_consistent"], r["root_ok"]])


def case_group_repair(res, which):
    """a bad job lists columns overwritten with all-ones words (mended: the undamaged columns), or lists
    one and holds an all-ones word in a column it does not list (refused); the others list nothing"""
    sound = stored_fleet(which)
    files = [(img.copy(), tree, pre, enc, rows, cap) for img, tree, pre, enc, rows, cap in sound]
    bads, expect = [], []
    for j, (img, tree, pre, enc, rows, cap) in enumerate(files):
        if not is_bad(which, j):
            bads.append([])
            expect.append("clean")
            continue
        el = img.view("<u8").reshape(enc, cap)
        if (j // 3) % 2 == 0:
            n = min(enc - pre, 3)
            bad = sorted({(7 * j + 3 * k) % enc for k in range(n)})
            el[bad, :] = FF
            expect.append("mended")
        else:
            bad = [(7 * j) % enc]
            el[bad, :] = FF
            if rows:
                el[(7 * j + 1) % enc, rows - 1] = FF
            expect.append("refused" if rows else "mended")
        bads.append(bad)
    no_single(*pos.repair_plan([f[4] for f in files], [f[2] for f in files], [f[3] for f in files],
                               [len(b) for b in bads]))
    out = pos.repair_files_grouped([f[0] for f in files], [f[2] for f in files], [f[3] for f in files],
                                   [f[4] for f in files], [f[5] for f in files], bads,
                                   [f[1][:f[3]] for f in files], want_tree=True)
    for j, (r, f, s, bad, e) in enumerate(zip(out, files, sound, bads, expect)):
        enc, rows, cap = f[3], f[4], f[5]
        if e == "refused":
            assert r["status"] == UNRECOVERABLE and r["cols"] is None, j
            res.add(f"status_{j}", r["status"])
            continue
        assert r["status"] == 0, (j, e)
        assert np.array_equal(r["cols"], s[0].view("<u8").reshape(enc, cap)[bad, :rows].reshape(len(bad), rows)), (j, e)
        assert np.array_equal(r["digests"], s[1][bad].reshape(len(bad), 32)), (j, e)
        assert np.array_equal(r["tree"], s[1]) and r["root"] == s[1][-1].tobytes(), (j, e)
        for k in ("cols", "digests", "tree"):
            res.add(f"{k}_{j}", r[k])


def audit_fleet(which):
    """(bytes, pre, enc, rows) at the widths the grouped contraction takes, never empty"""
    out = []
    for j in range(FLEET_N):
        pre, enc = AUDIT_DIMS[j % len(AUDIT_DIMS)]
        rows = max(FLEET_ROWS[j % len(FLEET_ROWS)], 1)
        out.append((file_bytes(which, 2000 + j, rows * 7 * pre - 3), pre, enc, rows))
    return out


def case_group_audit(res, which):
    """answer_evaluation_requests' device work: the grouped u^T M over the raw files, then one encode"""
    files = audit_fleet(which)
    datas, pres = [f[0] for f in files], [f[1] for f in files]
    tiles, launches = pos.left_multiply_group_plan([d.size for d in datas], pres)
    no_single(tiles, launches)
    rng = np.random.default_rng(seed_of(which, 2100))
    lefts = [rng.integers(0, P63, f[3], dtype=np.uint64) for f in files]
    out = pos.left_multiply_unencoded_matrices_by_vectors(datas, pres, lefts)
    for j, (v, f) in enumerate(zip(out, files)):
        if j % 6 == 0:
            one = pos.left_multiply_unencoded_matrix_by_vector(f[0].tobytes(), f[1], lefts[j])
            assert np.array_equal(v.reshape(-1), np.asarray(one).reshape(-1)), j
        res.add(f"vector_{j}", v)


def case_group_verify(res, which):
    """36 audit responses; a bad one has a wrong column word (its leaf no longer reaches the root: paths), a
    wrong path digest (paths) or a wrong result word (values), by turns"""
    audits, expect = [], []
    for j in range(FLEET_N):
        pre, enc = FLEET_DIMS[j % len(FLEET_DIMS)]
        rows = max(FLEET_ROWS[j % len(FLEET_ROWS)], 1)
        n = rows * pre - (1 if pre > 2 else 0)
        code = L.LigeroEncoding.new_from_dims(FT63, pre, enc)
        comm = L.LcCommit.commit(L.field_random(FT63, n, seed_of(which, 3000 + j)), code)
        point = L.field_random(FT63, 1, seed_of(which, 3100 + j))
        left, _ = pos.form_side_vectors_for_polynomial_evaluation_from_point(point, rows, pre)
        result = np.array(pos.verifiable_polynomial_evaluation(comm, left), np.uint64).copy()
        cols = sorted({(3 * j + 5 * k) % enc for k in range(min(enc, 1 + j % 5))})
        opened = comm.open_columns(cols)
        if not is_bad(which, j):
            expect.append(None)
        else:
            kind = (j // 3) % 3
            if kind == 0:
                col = np.array(opened[0].col, np.uint64).copy()
                col.reshape(-1)[rows - 1] ^= np.uint64(2)
                opened[0] = L.LcColumn(col, opened[0].path)
            elif kind == 1:
                path = list(opened[-1].path)
                path[0] = bytes([path[0][0] ^ 0x40]) + path[0][1:]
                opened[-1] = L.LcColumn(opened[-1].col, path)
            else:
                result.reshape(-1)[cols[0]] ^= np.uint64(1)
            expect.append("values" if kind == 2 else "paths")    # (a wrong column word changes its leaf)
        audits.append((comm.get_root(), 7 * n, pre, enc, point, cols, result, opened))
    tiles, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    no_single(tiles, launches)
    out = pos.client_verify_evaluations_grouped(audits)
    for j, (g, e) in enumerate(zip(out, expect)):
        if e is None:
            assert isinstance(g, np.ndarray), (j, g)
            res.add(f"value_{j}", g)
        else:
            assert isinstance(g, L.VerifierError) and e in str(g), (j, e, g)
            res.add(f"verdict_{j}", e)


def case_sharded(res, which, hm):
    from lcpc_proof_of_storage_amd import shard
    enc = L.RsEncoding.new(FT127, 256, 512, 24, 2)
    polys = [L.field_random(FT127, 64 * 256, seed_of(which, 4000 + k)) for k in range(4)]
    ds = [hm.to_device(p) for p in polys]
    try:
        roots, proofs = shard.sharded_commit_prove_many(enc, shard.NativeComm.single(), ds, 64,
                                                        L.field_random(FT127, 64, seed_of(which, 4010)),
                                                        lambda i, root: tr(root))
    finally:
        for d in ds:
            hm.free(d)
    for k, (root, pf, poly) in enumerate(zip(roots, proofs, polys)):
        assert root == L.LcCommit.commit(poly, enc).get_root(), k
        res.add(f"root_{k}", root)
        res.add(f"proof_{k}", pf.to_bincode())


# ---------------------------------------------------------------- driver
def run_case(name, which, keep, hm, tmp):
    res = Result(name, keep)
    if name == "ligero_device_f1":
        case_ligero_device(res, which, hm)
    elif name == "ligero_fused_f1":
        case_ligero_fused(res, which, hm)
    elif name.startswith("ligero_f"):
        case_ligero(res, which, int(name[-1]))
    elif name.startswith("sdig_f"):
        case_sdig(res, which, int(name[-1]))
    elif name.startswith("batch_f"):
        case_batch(res, which, int(name[-1]))
    elif name.startswith("digest_"):
        case_digest(res, which, L.SHA256 if name == "digest_sha256" else L.SHA3_256)
    elif name.startswith("decoders_"):
        _, f, n, m = name.split("_")
        case_decoders(res, which, int(f[1:]), int(n), int(m))
    elif name.startswith("files_"):
        _, p, e, c = name.split("_")
        case_files(res, which, int(p), int(e), c == "cache", tmp)
    elif name == "sharded_n1":
        case_sharded(res, which, hm)
    else:
        globals()["case_" + name](res, which)
    return res


def probe():
    """the allocator's own selftest: a fresh block and a recycled one of every size, with and without a stream"""
    out = []
    for n in (256, 4096, (1 << 20) + 1):
        for with_stream in (True, False):
            for _ in range(2):
                out.append(dict(L.selftest_pool_poison(n, with_stream), bytes=n, with_stream=with_stream))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--order", choices=["ab", "b"], default="ab")
    ap.add_argument("--parts")
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--keep-going", action="store_true", help="go on after a case's failed assertion; exit 2 at the end")
    ap.add_argument("--only", help="a comma-separated subset of the cases (for working on one)")
    args = ap.parse_args()
    assert L.device_count() > 0, "no HIP device"
    L.set_device(0)
    if args.probe:
        return probe()
    from conftest import _HipMem
    hm = _HipMem()
    names = CASES if not args.only else [c for c in CASES if c in args.only.split(",")]
    out, parts, failed = {}, {}, []
    tmp = tempfile.mkdtemp(prefix="pool_poison_")
    t0 = time.perf_counter()
    try:
        for which in ("A", "B") if args.order == "ab" else ("B",):
            for name in names:
                print(f"case {which} {name}", file=sys.stderr, flush=True)
                try:
                    res = run_case(name, which, which == "B" and bool(args.parts), hm, tmp)
                except (AssertionError, L.LcpcError, PF.UnrecoverableError) as e:
                    # (a device error always ends the run; a refusal is a verdict like any other)
                    if not args.keep_going or (isinstance(e, L.LcpcError) and not isinstance(e, L.VerifierError)
                                               and e.code != UNRECOVERABLE):
                        raise
                    import traceback
                    traceback.print_exc()
                    failed.append(f"{which} {name}")
                    continue
                if which == "B":
                    out[name] = res.h.hexdigest()
                    parts.update(res.parts)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(f"done in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    if args.parts:
        np.savez(args.parts, **parts)
    print(json.dumps(out))
    if failed:
        print(f"failed: {failed}", file=sys.stderr)
        sys.exit(2)


if __name__ == "__main__":
    main()
