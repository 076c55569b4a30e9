"""CPU: the mutation builder (verify_mut.py) against the oracle alone.  Every mutation class gets from
the oracle (the C verifier, batch_ref.verify_batch) the verdict it was built for -- RAW ColumnDegree
(ColumnEval without degree tests), DEGREE_BLIND ColumnEval, ALL_BLIND ColumnPath, path and root flips
ColumnPath -- and the untouched proof verifies, on the smallest and the largest shape of the GPU
sweeps' tables, all five fields.  This keeps the GPU sweeps (test_gpu_verify_sweep.py) from quietly
degenerating: the count of generated cases per class is asserted from the place lists, so a class may
only leave out a column too short for it (n_rows < n_degree_tests + 1 resp. + 2, the one-row shape)."""
import collections

import numpy as np
import pytest

import verify_mut as V

FT63, FT127, FT191, FT255, FT253_192 = V.FIELD_IDS


def test_place_lists():
    """the lists by hand at a few shapes"""
    assert V.opened_places(70, 1) == [0, 1, 62, 63, 64, 65, 69]
    assert V.opened_places(70, 2) == [0, 1, 31, 32, 62, 63, 64, 65, 69]
    assert V.opened_places(70, 4) == [0, 1, 15, 16, 62, 63, 64, 65, 69]
    assert V.opened_places(70, 5) == [0, 1, 12, 62, 63, 64, 65, 69]   # flags 60..64 are column 12's
    assert V.opened_places(6, 2) == [0, 1, 5]
    # Ft63: 8-byte elements after 32 zero bytes: rows 0..123 in chunk 0, 124..251 in chunk 1
    assert [V.rows_for_chunks(FT63, c) for c in (1, 2, 3, 9, 17)] == [124, 125, 253, 1021, 2045]
    assert V.chunk_rows(FT63, 125) == [(0, 123), (124, 124)]
    assert V.row_places(FT63, 125) == [0, 1, 3, 4, 123, 124]
    assert V.row_places(FT63, 253) == [0, 1, 3, 4, 123, 124, 251, 252]
    # Ft191: 24-byte elements; row 41 holds words 254..259 and straddles chunks 0 and 1
    assert [V.rows_for_chunks(FT191, c) for c in (1, 2, 3, 9, 17)] == [41, 42, 85, 341, 682]
    assert V.chunk_rows(FT191, 42) == [(0, 41), (41, 41)]
    assert V.chunk_rows(FT191, 85) == [(0, 41), (41, 83), (84, 84)]
    assert V.row_places(FT191, 85) == [0, 1, 41, 83, 84]             # row 1 holds words 14..19: both sides
    assert [V.rows_for_chunks(FT255, c) for c in (1, 2, 3)] == [31, 32, 64]
    assert V.row_places(FT255, 64) == [0, 1, 30, 31, 62, 63]
    assert all(V.n_chunks(f, V.rows_for_chunks(f, c)) == c and (c == 1 or V.n_chunks(f, V.rows_for_chunks(f, c) - 1) == c - 1)
               for f in V.FIELD_IDS for c in V.CHUNK_CLASSES[f])
    assert len(V.row_places(FT63, 2045, thin=True)) == 2 * 17 - 1   # the last chunk's one row is first and last
    assert V.word_rows(FT127, 127) == [61, 125, 126]


def test_blind_is_exact_and_moves_past_singular_helper_rows():
    p = 2**61 - 1
    vs = [[3, 1, 4, 1, 5, 9], [2, 7, 1, 8, 2, 8]]
    d = V.blind(vs, 2, 5, 6, p)
    assert d[2] == 5 and sum(1 for x in d if x) <= 3 and all(V.dot(v, d, p) == 0 for v in vs)
    # rows 3 and 4 are proportional in both vectors: that window is singular, the next one is not
    vs = [[1, 2, 3, 1, 2, 5], [4, 5, 6, 3, 6, 1]]
    d = V.blind(vs, 2, 1, 6, p)
    assert d[2] == 1 and d[3] == 0 and all(V.dot(v, d, p) == 0 for v in vs)
    with pytest.raises(ValueError):
        V.blind(vs, 0, 1, 2, p)
    with pytest.raises(ArithmeticError):
        V.blind([[1, 0, 0]], 0, 1, 3, p)


def _check(case):
    ctx = V.oracle_context(case)
    shape, fid, ndt, m = case["shape"], case["fid"], case["ndt"], case["m"]
    kind, evs = V.oracle_verdict(ctx, ctx.proof)
    assert kind == V.OK and len(evs) == m
    assert ctx.ndt == ndt and ctx.m == m and ctx.idx == list(ctx.proof.col_idx)
    seen, per_place = collections.Counter(), collections.Counter()
    for mut in V.sweep(ctx, shape):
        seen[mut.cls] += 1
        kind, _ = V.verdict(ctx, mut)
        # the full verify of the whole proof: every mutation of the one-row proof; of the others the
        # first three per (class, opened column), the root's first and last byte, and all that
        # verdict() does not shorten anyway
        per_place[(mut.cls, mut.k)] += 1
        if shape.n_rows == 1 or per_place[(mut.cls, mut.k)] <= 3 or mut.where == "root byte 31":
            assert V.verdict(ctx, mut, full=True)[0] == kind, (mut.cls, mut.where)
        if mut.expect is not None:
            assert kind == mut.expect, (mut.cls, mut.where, V.KIND.get(kind, kind))
        elif mut.cls in (V.P_EVAL, V.P_RANDOM):
            assert kind != V.OK, (mut.cls, mut.where)
    want = V.sweep_counts(fid, shape, ndt, m)
    assert {c: seen[c] for c in want} == want
    assert seen[V.EXCHANGE] >= 2
    short = shape.n_rows == 1
    assert (want[V.ALL_BLIND] == 0) == short and (want[V.DEGREE_BLIND] == 0) == (short and ndt > 0)
    assert want[V.RAW] > 0 and want[V.PATH] > 0


@pytest.mark.parametrize("ndt", V.NDTS)
@pytest.mark.parametrize("which", ["smallest", "largest"])
@pytest.mark.parametrize("fid", V.FIELD_IDS)
def test_single_proof_mutations_get_their_verdict(fid, which, ndt):
    shape = V.ONE_ROW if which == "smallest" else V.single_shapes(fid, V.CHUNK_CLASSES[fid][-1])[0]
    _check(V.oracle_case(fid, shape, ndt))


@pytest.mark.parametrize("ndt", V.BATCH_NDTS)
@pytest.mark.parametrize("m", V.BATCH_MS)
@pytest.mark.parametrize("fid", V.BATCH_FIELDS)
def test_batch_proof_mutations_get_their_verdict(fid, m, ndt):
    _check(V.oracle_case(fid, V.batch_shape(fid), ndt, m))


def test_value_shift_stays_reduced():
    import oracle_ffi as O
    for fid in V.FIELD_IDS:
        p = O.modulus(fid)
        for v in (0, 1, p - 1, p >> 1):
            e = O.to_mont(fid, [v])
            for w in range(V.field_words(fid)):
                got = V.canon(fid, V.shift_value(fid, e, w, p))[0]
                assert got < p and abs(got - v) == 1 << (32 * w)
                stored = V.stored_int(fid, V.shift_stored(fid, e, w, p))
                assert stored < p and abs(stored - V.stored_int(fid, e)) == 1 << (32 * w)
            assert V.canon(fid, V.other_element(fid, e, p))[0] == (v + 1) % p
    assert np.array_equal(V.add_delta(0, O.to_mont(0, [5, 6]), [0, 0], O.modulus(0)), O.to_mont(0, [5, 6]))
