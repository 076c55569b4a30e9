"""GPU: the grouped check of stored-file audit responses --
lcpc_pos_verify_evaluations_grouped (csrc/pos_verify_group.hip, pos_verify_group_host.cpp) behind
pos.client_verify_evaluations_grouped.  The reference of every comparison is the single check
(pos.client_verify_evaluation, the code the update audits have always run), never the grouped path
itself: a passing job's evaluation is compared word for word, a failing job's VerifierError by its
kind and by whether it names the paths or the values.  For tampered responses the verdict is also
known by construction.  All comparisons are exact.

Honest responses are built in memory: random field elements committed under (pre, enc), the columns
opened with their paths, the result vector u^T Enc(M) for the left side vector of the point."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FT63 = 0
P = 5102708120182849537
REGION = "pos_group_verify"
# the row counts at which a column's leaf (32 zero bytes, then 8 bytes per row, 1-KiB chunks) goes
# from 1 to 2, 2 to 3, 3 to 4, 4 to 5 and 5 to 6 chunks, and where the first block is exactly full
ROWS = (1, 3, 4, 5, 124, 125, 252, 253, 380, 381, 508, 509, 637)


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


class Server:
    """Honest responses, the commitments kept: one commit per (elements, pre, enc, seed)."""

    def __init__(self, gpu, pos):
        self.gpu, self.pos, self.commits = gpu, pos, {}

    def commit(self, n_elems, pre, enc, seed):
        key = (n_elems, pre, enc, seed)
        if key not in self.commits:
            code = self.gpu.LigeroEncoding.new_from_dims(FT63, pre, enc)
            self.commits[key] = self.gpu.LcCommit.commit(self.gpu.field_random(FT63, n_elems, 1000 + seed), code)
        return self.commits[key]

    def audit(self, n_elems, pre, enc, seed, point, cols):
        """(root, file_len, pre, enc, point, cols, result_vector, columns) of an honest server"""
        comm = self.commit(n_elems, pre, enc, seed)
        n_rows = -(-n_elems // pre)
        left, _ = self.pos.form_side_vectors_for_polynomial_evaluation_from_point(point, n_rows, pre)
        result = self.pos.verifiable_polynomial_evaluation(comm, left)
        cols = sorted(int(c) for c in cols)
        return (comm.get_root(), 7 * n_elems, pre, enc, point, cols, result, comm.open_columns(cols))


@pytest.fixture(scope="module")
def server(gpu, pos):
    return Server(gpu, pos)


def elems(rows, pre):
    """an element count with `rows` rows of pre, the last row short for some"""
    return rows * pre - (rows % 3 if pre > 2 else 0)


def fleet(gpu, server, seed, specs):
    """audits for specs = [(rows, pre, enc, n_cols), ...]: a point and the columns drawn per job"""
    rng = np.random.default_rng(seed)
    points = gpu.field_random(FT63, len(specs), seed)
    out = []
    for k, (rows, pre, enc, n_cols) in enumerate(specs):
        cols = rng.choice(enc, size=n_cols, replace=False).tolist() if n_cols else []
        out.append(server.audit(elems(rows, pre), pre, enc, rows % 5, points[k:k + 1], cols))
    return out


def single(gpu, pos, audit):
    try:
        return pos.client_verify_evaluation(*audit)
    except gpu.VerifierError as e:
        return e


def names(err):
    text = str(err).lower()
    return "paths" if "path" in text else "values" if "value" in text else text


def same(gpu, got, want, where=""):
    if isinstance(want, Exception):
        assert isinstance(got, gpu.VerifierError), (where, got, want)
        assert got.kind == want.kind == "ColumnEval" and names(got) == names(want), (where, got, want)
    else:
        assert isinstance(got, np.ndarray), (where, got)
        assert got.shape == want.shape and got.dtype == want.dtype, where
        assert np.array_equal(got, want), (where, got, want)


def check(gpu, pos, audits, sample=None):
    """grouped against the single check, job by job (or on `sample`); returns the grouped list"""
    got = pos.client_verify_evaluations_grouped(audits)
    assert len(got) == len(audits)
    for j in (range(len(audits)) if sample is None else sample):
        same(gpu, got[j], single(gpu, pos, audits[j]), f"job {j}")
    return got


def with_column(audit, k, col=None, path=None):
    from lcpc_proof_of_storage_amd import LcColumn
    columns = list(audit[7])
    columns[k] = LcColumn(columns[k].col.copy() if col is None else col, list(columns[k].path) if path is None else path)
    return audit[:7] + (columns,)


def with_result(audit, result):
    return audit[:6] + (result, audit[7])


def test_every_chunk_count_at_the_smallest_dims(gpu, pos, server):
    """Every row count of ROWS at pre = 8, enc = 16 in one call, with 1, 5 and all 16 columns opened:
    one- to six-chunk leaves side by side, odd row counts (the zero pad of a column's stride)."""
    specs = [(r, 8, 16, n) for r in ROWS for n in (1, 5, 16)]
    got = check(gpu, pos, fleet(gpu, server, 1, specs))
    assert all(isinstance(g, np.ndarray) for g in got)


def test_column_counts_around_a_wave(gpu, pos, server):
    """1, 63, 64, 65 and all enc = 256 columns of a job: one wave, a full one, a second wave with one lane."""
    specs = [(3, 64, 256, n) for n in (1, 63, 64, 65, 256)] + [(125, 64, 256, 65), (4, 64, 256, 256)]
    got = check(gpu, pos, fleet(gpu, server, 2, specs))
    assert all(isinstance(g, np.ndarray) for g in got)


def test_mixed_dims_two_points_and_no_columns(gpu, pos, server):
    """Five dims in one call (a decode per distinct enc, an encode per distinct dims), the same file at
    two points, and jobs that open no column: their value is still returned."""
    dims = [(8, 16), (16, 32), (24, 32), (64, 256), (16, 64)]
    specs = [(r, pre, enc, n) for (pre, enc), r, n in zip(dims * 3, (5, 125, 3, 9, 253, 1, 4, 126, 2, 7, 3, 381, 6, 124, 11),
                                                         (3, 7, 0, 20, 9, 2, 16, 1, 5, 0, 4, 8, 31, 6, 64))]
    audits = fleet(gpu, server, 3, specs)
    again = server.audit(elems(125, 16), 16, 32, 125 % 5, gpu.field_random(FT63, 1, 77), [0, 9, 31])
    audits.insert(4, again)
    got = check(gpu, pos, audits)
    assert all(isinstance(g, np.ndarray) for g in got)
    assert audits[1][0] == audits[4][0] and not np.array_equal(got[1], got[4])   # one file, two points
    empty = [a for a in audits if not a[5]]
    assert len(empty) == 2
    for g, a in zip(pos.client_verify_evaluations_grouped(empty), empty):
        same(gpu, g, single(gpu, pos, a))


def test_one_job_alone(gpu, pos, server):
    check(gpu, pos, fleet(gpu, server, 4, [(253, 8, 16, 7)]))


def test_three_hundred_jobs_in_one_launch(gpu, pos, server):
    """300 responses over a few files: one staging group, and the grouped region is entered as often as
    the plan has launches, not once per job.  The single checks are made on a SAMPLE of 60 jobs (the
    first, the last and 58 drawn), the rest only has to pass."""
    shapes = [(r, 8, 16) for r in (1, 4, 125, 253)] + [(3, 16, 32), (126, 16, 64), (9, 64, 256)]
    rng = np.random.default_rng(300)
    specs = [shapes[j % len(shapes)] + (int(rng.integers(1, 12)),) for j in range(300)]
    audits = fleet(gpu, server, 5, specs)
    _, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    assert launches == 1
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = pos.client_verify_evaluations_grouped(audits)
        _, count = gpu.prof_stats().get(REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert count == launches
    assert all(isinstance(g, np.ndarray) for g in got)
    sample = sorted({0, 299} | set(rng.choice(np.arange(1, 299), size=58, replace=False).tolist()))
    assert len(sample) == 60
    for j in sample:
        same(gpu, got[j], single(gpu, pos, audits[j]), f"job {j}")


def test_three_staging_groups_and_a_job_above_the_group(gpu, pos, server, monkeypatch):
    """With the staging seam at 8 KiB, jobs of 2000 column bytes fill three groups, so both page-locked
    blocks are reused; between two small jobs, one whose columns exceed the group goes through the
    single sequence inside the same call."""
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", "8192")
    specs = [(125, 8, 16, 2)] * 5 + [(253, 8, 16, 16)] + [(124, 8, 16, 2), (5, 8, 16, 3)] * 3 + [(125, 16, 32, 2)] * 2
    audits = fleet(gpu, server, 6, specs)
    tiles, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    assert sorted(set(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE])) == [5]
    assert launches >= 3
    got = check(gpu, pos, audits)
    assert all(isinstance(g, np.ndarray) for g in got)


def group_first_jobs(tiles):
    """the first job of every launch of a plan"""
    return {int(tiles["job"][tiles["launch"] == n].min()) for n in set(tiles["launch"].tolist())}


@pytest.mark.parametrize("places", [(0, 1, 2), (36, 38, 39), (4, 3, 5)], ids=["first", "last", "boundary"])
def test_tampered_responses_among_honest_ones(gpu, pos, server, monkeypatch, places):
    """40 jobs, exactly 3 altered: a bit of a column's last element at a job with a 3-chunk leaf and a
    swapped path sibling must report the paths, a result vector replaced by another codeword passes the
    paths and must report the values.  The other 37 equal the single check, wherever the three sit:
    first, last, or at a group boundary (the seam at 16 KiB: every four jobs are a staging group, job 3
    ends the first and job 4 opens the second)."""
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", "16384")
    cycle = [(253, 8, 16, 4), (5, 8, 16, 3), (124, 16, 32, 5), (9, 8, 16, 16)]
    audits = fleet(gpu, server, 7, [cycle[j % 4] for j in range(40)])
    tiles, launches = pos.verify_group_plan([a[1] for a in audits], [a[2] for a in audits], [len(a[5]) for a in audits])
    assert launches == 10 and group_first_jobs(tiles) == set(range(0, 40, 4))
    a, b, c = places
    assert (tiles["job"] == a).sum() == 3   # one wave of columns, three chunks
    col = audits[a][7][2].col.copy()
    col.reshape(-1)[-1] ^= np.uint64(1 << 17)
    audits[a] = with_column(audits[a], 2, col=col)
    path = list(audits[b][7][1].path)
    path[0], path[1] = path[1], path[0]
    assert path != list(audits[b][7][1].path)
    audits[b] = with_column(audits[b], 1, path=path)
    other = server.audit(audits[c][1] // 7, audits[c][2], audits[c][3], 3, gpu.field_random(FT63, 1, 99), [0])
    assert not np.array_equal(other[6], audits[c][6])
    audits[c] = with_result(audits[c], other[6])
    got = check(gpu, pos, audits)
    assert names(got[a]) == "paths" and names(got[b]) == "paths" and names(got[c]) == "values"
    assert sum(isinstance(g, np.ndarray) for g in got) == 37


def test_words_outside_the_field_and_non_codewords(gpu, pos, server):
    """Untrusted words: a result vector changed at a position that is not opened, and the words p, p + 1
    and 2^64 - 1 inside a column and inside a result vector.  Whatever the single check says, the
    grouped check says."""
    base = fleet(gpu, server, 8, [(125, 8, 16, 4), (5, 16, 32, 6), (253, 8, 16, 3)])
    audits = list(base)
    for a in base:
        res = np.array(a[6], copy=True)
        closed = [i for i in range(a[3]) if i not in a[5]]
        res.reshape(-1)[closed[1]] ^= np.uint64(5)
        audits.append(with_result(a, res))
        for w in (P, P + 1, 2**64 - 1):
            col = a[7][0].col.copy()
            col.reshape(-1)[col.size // 2] = np.uint64(w)
            audits.append(with_column(a, 0, col=col))
            res = np.array(a[6], copy=True)
            res.reshape(-1)[a[5][0]] = np.uint64(w)
            audits.append(with_result(a, res))
            res = np.array(a[6], copy=True)
            res.reshape(-1)[closed[0]] = np.uint64(w)
            audits.append(with_result(a, res))
    check(gpu, pos, audits)


def test_shape_failures_stay_with_their_entry(gpu, pos, server):
    """A short column, a missing path digest and a result of enc - 1 words are that entry's
    VerifierError; the neighbours still verify.  Non-increasing columns are the caller's mistake."""
    from lcpc_proof_of_storage_amd import LcColumn
    audits = fleet(gpu, server, 9, [(5, 8, 16, 4)] * 7)
    short = audits[1][7][0]
    audits[1] = with_column(audits[1], 0, col=short.col[:-1].copy())
    audits[3] = with_column(audits[3], 2, path=list(audits[3][7][2].path)[:-1])
    audits[5] = with_result(audits[5], np.asarray(audits[5][6]).reshape(-1)[:-1].copy())
    got = check(gpu, pos, audits)
    for j in range(7):
        assert isinstance(got[j], gpu.VerifierError if j in (1, 3, 5) else np.ndarray), j
    fewer = audits[0][:7] + (list(audits[0][7])[:-1],)
    assert isinstance(pos.client_verify_evaluations_grouped([fewer, audits[2]])[0], gpu.VerifierError)
    bad = audits[0][:5] + (list(reversed(audits[0][5])),) + audits[0][6:]
    with pytest.raises(ValueError):
        pos.client_verify_evaluations_grouped([audits[2], bad])
    with pytest.raises(ValueError):
        pos.client_verify_evaluation(*bad)
    assert isinstance(LcColumn, type) and pos.client_verify_evaluations_grouped([]) == []


def test_two_threads_each_with_its_own_fleet(gpu, pos, server):
    fleets = [fleet(gpu, server, 10 + i, [((5, 8, 16, 3), (125, 16, 32, 9), (253, 8, 16, 2))[(j + i) % 3] for j in range(20)])
              for i in range(2)]
    want = [[single(gpu, pos, a) for a in f] for f in fleets]
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                got[i] = pos.client_verify_evaluations_grouped(fleets[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for j, (g, w) in enumerate(zip(got[i], want[i])):
            same(gpu, g, w, f"thread {i} job {j}")


def test_answers_of_stored_files_go_straight_into_the_grouped_check(gpu, pos, tmp_path):
    """answer_evaluation_requests over five stored files, its answers verified in one grouped call: all
    pass, with the single check's values."""
    from lcpc_proof_of_storage_amd import pos_files as PF
    shapes = [(7 * 8 * 3 - 2, 8, 16), (7 * 16 * 20, 16, 32), (5000, 64, 128), (7 * 64 * 9 - 11, 64, 256), (20000, 24, 32)]
    rng = np.random.default_rng(55)
    requests, meta = [], []
    points = gpu.field_random(FT63, len(shapes), 12)
    for i, (n, pre, enc) in enumerate(shapes):
        name = f"01VERIFY{i:018d}"
        src = tmp_path / f"{name}.bin"
        src.write_bytes(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        fh = PF.FileHandler.create_from_unencoded_file(name, str(src), pre, enc, directory=str(tmp_path / name))
        cols = sorted(rng.choice(enc, size=min(6 + i, enc // 2), replace=False).tolist())
        requests.append((fh, points[i:i + 1], cols))
        meta.append((fh.get_commit_root(), n, pre, enc, points[i:i + 1], cols))
    audits = [m + answer for m, answer in zip(meta, PF.answer_evaluation_requests(requests))]
    got = check(gpu, pos, audits)
    assert all(isinstance(g, np.ndarray) for g in got)
    import lcpc_proof_of_storage_amd as L
    assert L.client_verify_evaluations_grouped is pos.client_verify_evaluations_grouped
    assert L.client_verify_evaluation is pos.client_verify_evaluation is pos._checked_file_evaluation
    assert L.verify_group_plan is pos.verify_group_plan
