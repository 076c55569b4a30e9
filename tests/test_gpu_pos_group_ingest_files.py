"""GPU: stored files created many at a time (FileHandler.create_from_unencoded_files over
lcpc_pos_encode_files_grouped): every file on disk is byte for byte what a loop of
create_from_unencoded_file writes, and the three grouped legs -- ingest, audit, check -- meet end to end."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FT63 = 0
SIZES = (1000, 65536, 0, 300_001, 7 * 64 * 9 - 11)


@pytest.fixture(scope="module")
def PF(gpu):
    from lcpc_proof_of_storage_amd import pos_files
    return pos_files


@pytest.fixture(scope="module")
def pos(gpu):
    from lcpc_proof_of_storage_amd import pos as M
    return M


def make_specs(pos, directory, tag):
    """five raw files of different default dims, one of them empty (the dims of an empty file are chosen)"""
    rng = np.random.default_rng(17)
    specs, datas = [], []
    for i, n in enumerate(SIZES):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        pre, enc = pos.get_aspect_ratio_default_from_file_len(n)[:2] if n else (8, 16)
        src = os.path.join(directory, f"upload_{tag}_{i}.bin")
        with open(src, "wb") as f:
            f.write(data)
        specs.append((f"01HINGEST{i:017d}", src, pre, enc))
        datas.append(data)
    assert len({(s[2], s[3]) for s in specs}) >= 4
    return specs, datas


def listing(directory):
    out = {}
    for name in sorted(os.listdir(directory)):
        with open(os.path.join(directory, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.mark.parametrize("chunk_cache", [False, True])
def test_files_equal_the_loop(gpu, pos, PF, tmp_path, chunk_cache):
    loop_dir, group_dir = str(tmp_path / "loop"), str(tmp_path / "group")
    os.makedirs(loop_dir)
    os.makedirs(group_dir)
    specs, datas = make_specs(pos, str(tmp_path), "a")
    loop = [PF.FileHandler.create_from_unencoded_file(u, src, pre, enc, loop_dir, chunk_cache=chunk_cache)
            for u, src, pre, enc in specs]
    specs, _ = make_specs(pos, str(tmp_path), "b")
    handlers = PF.FileHandler.create_from_unencoded_files(specs, group_dir, chunk_cache=chunk_cache)
    want, got = listing(loop_dir), listing(group_dir)
    exts = {"porraw", "porenc", "portree", "meta"} | ({"porcv"} if chunk_cache else set())
    assert sorted(want) == sorted(got) and {n.rsplit(".", 1)[1] for n in got} == exts and len(got) == 5 * len(exts)
    for name in want:
        assert got[name] == want[name], name
    for fh, ref, data in zip(handlers, loop, datas):
        fh.verify_all_files_agree()
        assert fh.get_commit_root() == ref.get_commit_root() and fh.get_dimensions() == ref.get_dimensions()
        assert fh.get_total_data_bytes() == len(data)
    assert pos.commit_roots_of_files(datas, [s[2] for s in specs], [s[3] for s in specs]) == \
        [fh.get_commit_root() for fh in handlers]


def test_specs_are_checked_before_any_file_moves(pos, PF, tmp_path):
    d = str(tmp_path / "d")
    os.makedirs(d)
    specs, _ = make_specs(pos, str(tmp_path), "c")
    for bad in ((specs[4][0], specs[4][1], 8, 24), (specs[4][0], specs[4][1], 0, 16), (specs[4][0], specs[4][1], 16, 16),
                (specs[4][0], str(tmp_path / "missing.bin"), 8, 16), (specs[0][0], specs[4][1], 8, 16)):
        with pytest.raises((ValueError, FileNotFoundError)):
            PF.FileHandler.create_from_unencoded_files(specs[:4] + [bad], d)
        assert os.listdir(d) == [] and all(os.path.isfile(s[1]) for s in specs)
    assert PF.FileHandler.create_from_unencoded_files([], d) == []


def test_three_grouped_legs_end_to_end(gpu, pos, PF, tmp_path):
    d = str(tmp_path / "e2e")
    os.makedirs(d)
    specs, datas = make_specs(pos, str(tmp_path), "d")
    roots = pos.commit_roots_of_files(datas, [s[2] for s in specs], [s[3] for s in specs])   # the client, before upload
    handlers = PF.FileHandler.create_from_unencoded_files(specs, d)                           # the server
    live = [i for i, n in enumerate(SIZES) if n]
    rng = np.random.default_rng(3)
    points = gpu.field_random(FT63, len(live), 23)
    requests, audits = [], []
    for k, i in enumerate(live):
        enc = specs[i][3]
        cols = sorted(rng.choice(enc, size=min(8, enc // 2), replace=False).tolist())
        requests.append((handlers[i], points[k:k + 1], cols))
    answers = PF.answer_evaluation_requests(requests)
    for (fh, x, cols), (result, opened), i in zip(requests, answers, live):
        audits.append((roots[i], SIZES[i], specs[i][2], specs[i][3], x, cols, result, opened))
    verdicts = pos.client_verify_evaluations_grouped(audits)
    assert len(verdicts) == len(live) and all(isinstance(v, np.ndarray) for v in verdicts), verdicts
    # a response checked against another file's root fails: the roots are what the verdicts hang on
    swapped = [(roots[live[(k + 1) % len(live)]],) + a[1:] for k, a in enumerate(audits)]
    assert not any(isinstance(v, np.ndarray) for v in pos.client_verify_evaluations_grouped(swapped))
