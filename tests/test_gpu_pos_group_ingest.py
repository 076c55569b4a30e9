"""GPU: the grouped ingest of small files (lcpc_pos_encode_files_grouped) against the oracle
restatement of convert_unencoded_file (image, tree, rows) and against one lcpc_pos_encode_file per file
on identically prefilled buffers; the chaining values against a finalized writer's.  Every comparison is
exact."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REGION = "pos_group_ingest"
FILL = 0xA5
CUTS = (0, 1, 6, 7, 55, 56, 57)


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


@pytest.fixture(scope="module")
def native(gpu):
    from lcpc_proof_of_storage_amd import _native as N
    N.load()
    return N


def file_rows(n_bytes, pre):
    return -(-(-(-n_bytes // 7)) // pre)


def u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8)) if a.size else None


def random_file(seed, n_bytes):
    return np.random.default_rng(seed).integers(0, 256, n_bytes, dtype=np.uint8)


def single(native, data, pre, enc, cap):
    """lcpc_pos_encode_file into a prefilled image, and the chaining values of a finalized writer over the
    same file: (image, tree, rows, cvs)"""
    lib = native.load()
    data = np.ascontiguousarray(data)
    img = np.full(enc * cap * 8, FILL, np.uint8)
    tree = np.zeros((2 * enc - 1, 32), np.uint8)
    rows = C.c_size_t()
    assert lib.lcpc_pos_encode_file(u8(data), data.size, pre, enc, cap, u8(img), u8(tree), C.byref(rows)) == 0
    h = native.vp()
    assert lib.lcpc_pos_writer_new(pre, enc, None, 0, 0, C.byref(h)) == 0
    try:
        assert lib.lcpc_pos_writer_push_bytes(h, u8(data), data.size) == 0
        t2 = np.zeros((2 * enc - 1, 32), np.uint8)
        assert lib.lcpc_pos_writer_finalize(h, None, u8(t2), None, None) == 0
        cvs = np.zeros((lib.lcpc_pos_writer_n_chunks(h), enc, 32), np.uint8)
        assert lib.lcpc_pos_writer_copy_cvs(h, u8(cvs)) == 0
    finally:
        lib.lcpc_pos_writer_free(h)
    assert np.array_equal(t2, tree)
    return img, tree, rows.value, cvs


def check_fleet(pos, native, oracle, files, caps=None, against_oracle=True):
    """files: (data, pre, enc); every output of the grouped call against the single call (whole prefilled
    buffers, so rows past rows_written too) and the oracle"""
    datas, pres, encs = [f[0] for f in files], [f[1] for f in files], [f[2] for f in files]
    rows = [file_rows(len(d), p) for d, p in zip(datas, pres)]
    caps = caps or [2 * r + 3 for r in rows]
    imgs = [np.full(e * c * 8, FILL, np.uint8) for e, c in zip(encs, caps)]
    res = pos.encode_files_grouped_into(datas, pres, encs, imgs, caps, True, True, True)
    for j, (d, p, e) in enumerate(files):
        s_img, s_tree, s_rows, s_cvs = single(native, d, p, e, caps[j])
        o = res[j]
        assert o["rows_written"] == s_rows == rows[j], j
        assert np.array_equal(imgs[j], s_img), (j, p, e, rows[j])
        assert np.array_equal(o["tree"], s_tree), (j, p, e, rows[j])
        assert o["root"] == s_tree[-1].tobytes()
        assert o["cvs"].shape == s_cvs.shape and np.array_equal(o["cvs"], s_cvs), (j, p, e, rows[j])
        if against_oracle:
            o_img, o_tree, o_rows, _ = oracle.pos_encode_file(bytes(np.ascontiguousarray(d)), p, e, caps[j])
            written = np.frombuffer(o_img, "<u8").reshape(e, caps[j])[:, :o_rows]
            assert o_rows == s_rows
            assert np.array_equal(imgs[j].view("<u8").reshape(e, caps[j])[:, :o_rows], written), (j, p, e)
            assert o["tree"].tobytes() == o_tree, (j, p, e)
    return res


def test_every_length_the_kernel_dispatches(pos, native, oracle):
    files = []
    for le in range(1, 11):
        enc = 1 << le
        for pre in sorted({enc // 2, 1, enc - 1} | ({24} if enc == 32 else set())):
            files.append((random_file(1000 * le + pre, 9 * 7 * pre - (le % 7)), pre, enc))
    tiles, groups = pos.ingest_plan([len(f[0]) for f in files], [f[1] for f in files], [f[2] for f in files])
    assert groups == 1 and not (tiles["launch"] == pos.GROUP_SINGLE).any()
    check_fleet(pos, native, oracle, files)


@pytest.mark.parametrize("pre,enc", [(8, 16), (24, 32)])
def test_tile_and_chunk_seams(pos, native, oracle, pre, enc):
    """the tile height T the plan reports, and the rows at which a column's leaf gains a chunk (chunk c
    covers rows [128 c - 4, 128 c + 124)) up to the ninth: eight chunks are a merge group of the fold"""
    tiles, _ = pos.ingest_plan([7 * pre * 100], [pre], [enc])
    T = int((tiles["row_hi"] - tiles["row_lo"]).max())
    assert T == pos.INGEST_TILE_ROWS
    files = []
    for rows in (T - 1, T, T + 1, 124, 125, 252, 253, 1020, 1021):
        files.append((random_file(rows, rows * 7 * pre - 3), pre, enc))
    res = check_fleet(pos, native, oracle, files)
    assert [o["cvs"].shape[0] for o in res] == [1, 1, 1, 1, 2, 2, 3, 8, 9]


def test_padding_is_per_image(pos, native, oracle):
    pre, enc = 8, 16
    files = [(random_file(k, 5 * 7 * pre - k), pre, enc) for k in CUTS] + [(random_file(99, 1), pre, enc)]
    files += [(random_file(k + 50, 3 * 7 * 24 - k), 24, 32) for k in CUTS]
    for v in (0xFF, 0x00, 0x80):
        files.append((np.full(7 * pre * 9 + 5, v, np.uint8), pre, enc))
        files.append((np.full(7 * 100 * 3 - 1, v, np.uint8), 100, 256))
    check_fleet(pos, native, oracle, files)
    # images back to back in one host buffer (the next file's bytes are the neighbour), from an odd address
    sizes = [5 * 7 * pre - k for k in CUTS] + [1, 57]
    buf = random_file(7, 1 + sum(sizes))
    off, packed = 1, []
    for n in sizes:
        packed.append((buf[off:off + n], pre, enc))
        off += n
    assert any(f[0].ctypes.data & 7 for f in packed) and packed[0][0].ctypes.data & 1
    check_fleet(pos, native, oracle, packed)


def test_untouched_capacity_and_exact_capacity(pos, native, oracle):
    files = [(random_file(3, 7 * 24 * 11 - 2), 24, 32), (random_file(4, 7 * 128 * 74), 128, 256)]
    check_fleet(pos, native, oracle, files)                                    # capacity 2 rows + 3
    check_fleet(pos, native, oracle, files, caps=[11, 74], against_oracle=False)  # capacity == rows


def test_many_jobs_few_launches(gpu, pos, native, oracle):
    files = [(random_file(j, 56 - (j % 3)), 8, 16) for j in range(1000)]
    _, groups = pos.ingest_plan([len(f[0]) for f in files], [8] * 1000, [16] * 1000)
    assert groups == 1
    datas, pres, encs = [f[0] for f in files], [8] * 1000, [16] * 1000
    gpu.prof_enable(True)
    try:
        gpu.prof_reset()
        got = pos.encode_files_grouped(datas, pres, encs, want_cvs=True)
        ms, count = gpu.prof_stats().get(REGION, (0.0, 0))
    finally:
        gpu.prof_enable(False)
        gpu.prof_reset()
    assert 1 <= count <= groups
    # every 50th against the single call, all of them against each other through the roots
    for j in range(0, 1000, 50):
        s_img, s_tree, s_rows, s_cvs = single(native, datas[j], 8, 16, 1)
        img, tree, rows, cvs = got[j]
        assert rows == s_rows == 1 and np.array_equal(img.reshape(-1).view(np.uint8), s_img)
        assert np.array_equal(tree, s_tree) and np.array_equal(cvs, s_cvs)
    roots = pos.commit_roots_of_files(datas, pres, encs)
    assert roots == [g[1][-1].tobytes() for g in got]


def test_mixed_fleet_in_one_group(pos, native, oracle):
    rng = np.random.default_rng(257)
    dims = [(1, 2), (8, 16), (24, 32), (15, 16), (128, 256), (100, 256), (512, 1024), (1023, 1024), (3, 4)]
    files = []
    for j in range(257):
        pre, enc = dims[j % len(dims)]
        rows = int(rng.choice([0, 1, 7, 8, 9, 17]))
        files.append((random_file(j, max(rows * 7 * pre - int(rng.choice(CUTS)), 0)), pre, enc))
    _, groups = pos.ingest_plan([len(f[0]) for f in files], [f[1] for f in files], [f[2] for f in files])
    assert groups == 1
    check_fleet(pos, native, oracle, files, against_oracle=False)
    check_fleet(pos, native, oracle, files[:27])


def test_groups_and_routing(pos, native, oracle, monkeypatch):
    monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(1 << 20))
    big = (1 << 20) + 100
    files = [(random_file(j, 300_000 + 1000 * j), 128, 256) for j in range(9)]        # three to a group
    files.insert(4, (random_file(20, big), 128, 256))                                 # above the group
    files.insert(7, (random_file(21, 7 * 1024 * 5 - 1), 1024, 2048))                  # enc = 2048
    files.insert(2, (np.zeros(0, np.uint8), 8, 16))                                   # an empty file between two
    tiles, groups = pos.ingest_plan([len(f[0]) for f in files], [f[1] for f in files], [f[2] for f in files])
    routed = np.unique(tiles["job"][tiles["launch"] == pos.GROUP_SINGLE])
    assert groups >= 4 and list(routed) == [5, 8]
    res = check_fleet(pos, native, oracle, files, against_oracle=False)
    assert res[2]["rows_written"] == 0 and res[2]["cvs"].shape == (1, 16, 32)
    o_img, o_tree, o_rows, _ = oracle.pos_encode_file(b"", 8, 16, 3)
    assert o_rows == 0 and res[2]["tree"].tobytes() == o_tree


def test_outputs_a_la_carte(pos, native, oracle):
    files = [(random_file(j, 7 * 24 * (3 + j) - j), 24, 32) for j in range(6)]
    datas, pres, encs = [f[0] for f in files], [24] * 6, [32] * 6
    want = [single(native, d, 24, 32, file_rows(len(d), 24)) for d in datas]
    roots = pos.commit_roots_of_files(datas, pres, encs)
    assert roots == [w[1][-1].tobytes() for w in want]
    only_tree = pos.encode_files_grouped_into(datas, pres, encs, None, None, True, False, False)
    assert all(set(o) == {"rows_written", "tree"} and np.array_equal(o["tree"], w[1]) for o, w in zip(only_tree, want))
    # a porenc for every other job, chaining values for the others
    caps = [file_rows(len(d), 24) if j % 2 == 0 else 0 for j, d in enumerate(datas)]
    imgs = [np.full(32 * c * 8, FILL, np.uint8) if j % 2 == 0 else None for j, c in enumerate(caps)]
    res = pos.encode_files_grouped_into(datas, pres, encs, imgs, caps, False, True, [j % 2 == 1 for j in range(6)])
    for j, (o, w) in enumerate(zip(res, want)):
        assert o["root"] == w[1][-1].tobytes() and o["rows_written"] == w[2] and "tree" not in o
        if j % 2 == 0:
            assert np.array_equal(imgs[j], w[0]) and "cvs" not in o
        else:
            assert np.array_equal(o["cvs"], w[3])
    got = pos.encode_files_grouped(datas, pres, encs, want_porenc=False)
    assert all(g[0] is None and np.array_equal(g[1], w[1]) and g[2] == w[2] for g, w in zip(got, want))


def test_one_image_two_dims(pos, native, oracle):
    data = random_file(11, 7 * 64 * 9 - 4)
    check_fleet(pos, native, oracle, [(data, 64, 128), (data, 24, 32), (data, 64, 128), (data, 1, 2)])


def test_two_host_threads(pos, native, oracle):
    fleets = [[(random_file(100 * t + j, 7 * 24 * (5 + j) - t), 24, 32) for j in range(40)] for t in range(2)]
    want = [[single(native, d, p, e, file_rows(len(d), p)) for d, p, e in fl] for fl in fleets]
    got, errs = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                got[t] = pos.encode_files_grouped([f[0] for f in fleets[t]], [24] * 40, [32] * 40, want_cvs=True)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for t in range(2):
        for g, w in zip(got[t], want[t]):
            assert np.array_equal(g[0].reshape(-1).view(np.uint8), w[0]) and np.array_equal(g[1], w[1])
            assert g[2] == w[2] and np.array_equal(g[3], w[3])
