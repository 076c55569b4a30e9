"""GPU: grouped audits of stored files -- lcpc_pos_left_multiply_bytes_grouped[_device]
(csrc/pos_group.hip, pos_group_host.cpp) and pos_files.answer_evaluation_requests.  Every job is
compared with the single-file call on the same bytes, word for word, and the small and the extreme
images with Python integers as well (tests/pos_batch_ref.py).  All comparisons are exact."""
import threading

import numpy as np
import pytest

import pos_batch_ref as B

pytestmark = pytest.mark.gpu
FT63 = 0
P = B.P
CUTS = (0, 1, 6, 7, 55, 56, 57)
REGION = "pos_group_left_mul"


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


def file_rows(n_bytes, pre):
    return -(-(-(-n_bytes // 7)) // pre)


def make_fleet(seed, dims, fill=None):
    """(images, pres, lefts) for dims = [(n_bytes, pre), ...]: random bytes and random words below p"""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, n, dtype=np.uint8) if fill is None else np.full(n, fill, np.uint8) for n, _ in dims]
    pres = [p for _, p in dims]
    lefts = [rng.integers(0, P, file_rows(n, p), dtype=np.uint64) for n, p in dims]
    return images, pres, lefts


def singles(pos, images, pres, lefts):
    return [pos.left_multiply_unencoded_matrix_by_vector(a.tobytes(), p, lv).reshape(-1)
            for a, p, lv in zip(images, pres, lefts)]


def python_integers(images, pres, lefts):
    return [np.array(B.left_mul(a.tobytes(), p, [int(v) for v in lv]), np.uint64) for a, p, lv in zip(images, pres, lefts)]


def same(got, want):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (w.size, 1) and g.dtype == np.uint64, j
        assert np.array_equal(g.reshape(-1), w), j


def device_arena(images, head=0):
    """One arena, every byte that is no image 0xff: image j at an offset = 0 (j even) or 8 (j odd)
    mod 16, at least 8 bytes of 0xff before it and after the last."""
    offsets, cur = [], head
    for j, a in enumerate(images):
        off = (cur + 8 + 15) & ~15
        off += 8 if j % 2 else 0
        offsets.append(off)
        cur = off + a.size
    arena = np.full(cur + 64, 0xff, np.uint8)
    for off, a in zip(offsets, images):
        arena[off:off + a.size] = a
    return arena, offsets


def grouped_device(pos, hipmem, images, pres, lefts, arena=None, offsets=None):
    if arena is None:
        arena, offsets = device_arena(images)
    dev = hipmem.to_device(arena)
    try:
        return pos.left_multiply_device_arena_by_vectors(dev, offsets, [a.size for a in images], pres, lefts)
    finally:
        hipmem.free(dev)


def odd_address(data: np.ndarray) -> np.ndarray:
    buf = np.zeros(data.size + 17, np.uint8)
    start = 1 if buf.ctypes.data % 2 == 0 else 2
    view = buf[start:start + data.size]
    view[:] = data
    assert view.ctypes.data % 2 == 1
    return view


@pytest.mark.parametrize("pre", [8, 16, 64, 512])
def test_ragged_tails_in_a_device_arena(pos, hipmem, pre):
    """The padding rule: files that end k bytes before a row's end, and a 1-byte file, packed into one
    arena whose every other byte is 0xff, at offsets = 0 and = 8 (mod 16).  A kernel that read past
    an image's end would pick up the 0xff of the gap or the next file's bytes."""
    dims = [(rows * 7 * pre - k, pre) for rows in (1, 2, 9) for k in CUTS if rows * 7 * pre - k > 0] + [(1, pre)]
    images, pres, lefts = make_fleet(pre, dims)
    arena, offsets = device_arena(images)
    assert {o % 16 for o in offsets} == {0, 8}
    want = singles(pos, images, pres, lefts)
    same(grouped_device(pos, hipmem, images, pres, lefts, arena, offsets), want)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    if pre <= 16:
        for w, ref in zip(want, python_integers(images, pres, lefts)):
            assert np.array_equal(w, ref)
    # images back to back, no gap at all: the next file's bytes are the neighbour
    tight = [a[:a.size & ~7] for a in images if a.size >= 8]
    t_pres = [pre] * len(tight)
    t_lefts = [lv[:file_rows(a.size & ~7, pre)] for a, lv in zip(images, lefts) if a.size >= 8]
    t_off = np.concatenate([[0], np.cumsum([a.size for a in tight])[:-1]]).tolist()
    same(grouped_device(pos, hipmem, tight, t_pres, t_lefts, np.concatenate(tight + [np.full(64, 0xff, np.uint8)]), t_off),
         singles(pos, tight, t_pres, t_lefts))


def test_a_thousand_one_row_files_in_one_launch(gpu, pos, hipmem):
    """1000 files of one row of 8 elements (some a few bytes short): 64 jobs per wave, one launch.
    The grouped region's launch count is the plan's number of staging groups, not the job count."""
    dims = [(56 - (j % 5 if j % 3 == 0 else 0), 8) for j in range(1000)]
    images, pres, lefts = make_fleet(1000, dims)
    want = python_integers(images, pres, lefts)
    _, launches = pos.left_multiply_group_plan([n for n, _ in dims], pres)
    assert launches == 1
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts)
        ms, count = gpu.prof_stats().get(REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    same(got, want)
    assert 1 <= count <= launches
    same(grouped_device(pos, hipmem, images, pres, lefts), want)
    assert all(np.array_equal(a, b) for a, b in zip(singles(pos, images, pres, lefts), want))


def test_many_jobs_in_one_workgroup(pos, hipmem):
    """257 jobs of pre = 16 (two lanes each) with 1, 2 or 3 rows: a workgroup holds many jobs, and
    waves of different depths sit next to each other."""
    dims = [((1 + j % 3) * 7 * 16 - (j % 7), 16) for j in range(257)]
    images, pres, lefts = make_fleet(257, dims)
    want = singles(pos, images, pres, lefts)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    same(grouped_device(pos, hipmem, images, pres, lefts), want)


def test_split_jobs_next_to_unsplit_ones(pos, hipmem):
    """pre = 8 with 17 rows is three row splits (partials and the grouped fold) beside jobs that write
    their output directly; pre = 16384 with 9 rows spans 64 waves, two splits deep."""
    dims = [(7 * 8 * 17, 8), (7 * 8 * 8, 8), (7 * 8 * 3 - 2, 8), (7 * 16384 * 9 - 57, 16384), (7 * 64 * 100 - 7, 64),
            (7 * 8 * 17 - 55, 8), (7 * 256 * 16, 256), (7 * 16384 * 1, 16384)]
    tiles, launches = pos.left_multiply_group_plan([n for n, _ in dims], [p for _, p in dims])
    assert launches == 1 and (tiles["job"] == 0).sum() == 3 and (tiles["job"] == 1).sum() == 1
    assert (tiles["job"] == 3).sum() == 2 * (16384 // 8 // 64)
    images, pres, lefts = make_fleet(17, dims)
    want = singles(pos, images, pres, lefts)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    same(grouped_device(pos, hipmem, images, pres, lefts), want)
    for j in (0, 1, 2, 5):
        assert np.array_equal(want[j], python_integers(images[j:j + 1], pres[j:j + 1], lefts[j:j + 1])[0])


def test_other_widths_fall_back_in_the_middle(pos, hipmem):
    """pre = 24 (and 4, and 12) take the single call's pack-first path inside the grouped call; the
    jobs around them stay grouped and every result is in its place."""
    dims = [(7 * 8 * 5, 8), (7 * 24 * 5 - 3, 24), (7 * 16 * 9, 16), (100, 4), (7 * 12 * 2, 12), (7 * 64 * 3 - 1, 64)]
    tiles, launches = pos.left_multiply_group_plan([n for n, _ in dims], [p for _, p in dims])
    assert launches == 3 and sorted(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE]) == [1, 3, 4]
    images, pres, lefts = make_fleet(24, dims)
    want = singles(pos, images, pres, lefts)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    same(grouped_device(pos, hipmem, images, pres, lefts), want)
    for w, ref in zip(want, python_integers(images, pres, lefts)):
        assert np.array_equal(w, ref)


@pytest.mark.parametrize("group_bytes", [None, 1 << 20])
def test_odd_addresses_and_staging_groups(pos, monkeypatch, group_bytes):
    """Host images at odd addresses; a file one row longer than two staging groups among small ones
    (it takes the single-file path in the same call).  With the staging seam at 1 MiB the small
    files span several groups, so both page-locked blocks are reused."""
    if group_bytes:
        monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(group_bytes))
    gb = group_bytes or pos.GROUP_STAGE_BYTES
    pre_big = 1024
    small = [(7 * 64 * 37 - 5, 64), (7 * 8 * 2, 8), (300 * 1024 + 3, 256), (7 * 512 * 50, 512), (1, 8)]
    dims = small[:3] + [(2 * gb + 7 * pre_big, pre_big)] + small[3:]
    if group_bytes:
        dims += [(300 * 1024 + 8 * j, 128) for j in range(12)]
    images, pres, lefts = make_fleet(99, dims)
    images = [odd_address(a) for a in images]
    tiles, launches = pos.left_multiply_group_plan([n for n, _ in dims], pres)
    assert list(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE]) == [3]
    assert launches == (2 if not group_bytes else 6)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), singles(pos, images, pres, lefts))


@pytest.mark.parametrize("fill", [0xff, 0x00, 0x80])
def test_extreme_images_against_python_integers(pos, hipmem, fill):
    """All-0xff / 0x00 / 0x80 images against left words p - 1, 1 and R mod p (the Montgomery one):
    the largest products the lazy reduction sees, in every tile shape."""
    shapes = [(7 * 8 * 17, 8), (7 * 16 * 33 - 1, 16), (7 * 64 * 9 - 56, 64), (7 * 8 * 1, 8)]
    words = (P - 1, 1, B.R % P)
    dims = [s for s in shapes for _ in words]
    images, pres, _ = make_fleet(fill, dims, fill=fill)
    lefts = [np.full(file_rows(n, p), words[i % 3], np.uint64) for i, (n, p) in enumerate(dims)]
    want = python_integers(images, pres, lefts)
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    same(grouped_device(pos, hipmem, images, pres, lefts), want)
    assert all(np.array_equal(a, b) for a, b in zip(singles(pos, images, pres, lefts), want))


def test_the_same_image_in_two_jobs(pos, hipmem):
    rng = np.random.default_rng(2)
    image = rng.integers(0, 256, 7 * 32 * 19 - 4, dtype=np.uint8)
    other = rng.integers(0, 256, 500, dtype=np.uint8)
    images, pres = [image, other, image], [32, 8, 32]
    lefts = [rng.integers(0, P, file_rows(a.size, p), dtype=np.uint64) for a, p in zip(images, pres)]
    want = singles(pos, images, pres, lefts)
    assert not np.array_equal(want[0], want[2])
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres, lefts), want)
    arena, offsets = device_arena([image, other])
    same(grouped_device(pos, hipmem, images, pres, lefts, arena, [offsets[0], offsets[1], offsets[0]]), want)
    # and under another shape: the same bytes as rows of 8
    pres2 = [32, 8, 8]
    lefts2 = lefts[:2] + [rng.integers(0, P, file_rows(image.size, 8), dtype=np.uint64)]
    same(pos.left_multiply_unencoded_matrices_by_vectors(images, pres2, lefts2), singles(pos, images, pres2, lefts2))


def test_two_host_threads(pos):
    """Two host threads call the grouped entry at once on different fleets; each gets its own words."""
    fleets = [make_fleet(70, [(7 * 8 * (1 + j % 20), 8) for j in range(300)] + [(7 * 256 * 40 - 9, 256)] * 4),
              make_fleet(71, [(7 * 64 * (1 + j % 11) - j % 7, 64) for j in range(200)] + [(7 * 24 * 3, 24)])]
    want = [singles(pos, *f) for f in fleets]
    got, errors = [None, None], []

    def work(i):
        try:
            for _ in range(3):
                got[i] = pos.left_multiply_unencoded_matrices_by_vectors(*fleets[i])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        same(got[i], want[i])


def test_answer_evaluation_requests_equals_the_single_responses(gpu, pos, PF, tmp_path):
    """Five stored files of different dims, one of them asked twice (at another point and other
    columns): every grouped response is the single response bit for bit -- result vector, column
    values, paths -- and passes the client's check of a stored-file evaluation against the file's root."""
    shapes = [(7 * 8 * 3 - 2, 8, 16), (7 * 16 * 20, 16, 32), (5000, 64, 128), (7 * 64 * 9 - 11, 64, 256), (40000, 24, 32)]
    rng = np.random.default_rng(5)
    handlers, datas = [], []
    for i, (n, pre, enc) in enumerate(shapes):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        name = f"01GROUP{i:019d}"
        src = tmp_path / f"{name}.bin"
        src.write_bytes(data)
        handlers.append(PF.FileHandler.create_from_unencoded_file(name, str(src), pre, enc, directory=str(tmp_path / name)))
        datas.append(data)
    points = gpu.field_random(FT63, 6, 11)
    order = [0, 1, 2, 3, 4, 2]
    requests = []
    for k, i in enumerate(order):
        enc = shapes[i][2]
        cols = sorted(rng.choice(enc, size=min(6 + k, enc // 2), replace=False).tolist())
        requests.append((handlers[i], points[k:k + 1], cols))
    answers = PF.answer_evaluation_requests(requests)
    assert len(answers) == len(requests)
    values = []
    for (fh, x, cols), (result, opened), i in zip(requests, answers, order):
        want_result, want_opened = fh.polynomial_evaluation_response(x, cols)
        assert result.shape == want_result.shape and result.dtype == want_result.dtype
        assert np.array_equal(result, want_result)
        assert len(opened) == len(want_opened)
        for a, b in zip(opened, want_opened):
            assert np.asarray(a.col).shape == np.asarray(b.col).shape and np.array_equal(a.col, b.col)
            assert list(a.path) == list(b.path)
        n, pre, enc = shapes[i]
        values.append(pos._checked_file_evaluation(fh.get_commit_root(), n, pre, enc, x, cols, result, opened))
    assert not np.array_equal(values[2], values[5])   # the file asked twice: two points, two values
    assert PF.answer_evaluation_requests([]) == []
    import lcpc_proof_of_storage_amd as L
    assert L.answer_evaluation_requests is PF.answer_evaluation_requests
    assert L.left_multiply_unencoded_matrices_by_vectors is pos.left_multiply_unencoded_matrices_by_vectors
