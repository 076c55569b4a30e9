"""GPU: no result depends on what a recycled pool block held before.

Every device buffer comes from Device::alloc (csrc/host_internal.hpp), an exact-size cache that never
initialises a block; correctness rests on the memsets that clear what a kernel only accumulates into and
on every kernel writing every word it later reads.  The rest of the suite calls the same entries at the
same shapes in one process and compares grouped calls with single ones on the same bytes, so a forgotten
word still holds the right answer.  Here a child process (tests/_pool_poison_child.py: the switch is per
process and the blocks must be its own) runs every case on data set A and then on B -- same shapes, other
bytes, opposite verdicts -- and B's results must be what B alone gives, with the pool left alone and with
LCPC_POOL_POISON filling every block with 0x00, 0xff or 0xa5 first.  Every comparison is exact.

The time of each child run is printed (-s)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import _pool_poison_child as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("LCPC_POOL_POISON", "LCPC_NO_MFMA", "LCPC_STREAM_MODE", "LCPC_PRIORITY_STREAMS", "LCPC_HOST_WAIT", "LCPC_KECCAK",
         "LCPC_ROW1_PREFETCH", "LCPC_ROW1_GLDS", "LCPC_SHARD_BULK_STREAMS", "LCPC_POS_GROUP_BYTES", "LCPC_NTT_LEAF_FUSE", "LCPC_NTT_PERSIST",
         "LCPC_NTT_PERSIST_GRID", "LCPC_NTT_TW4")


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(HERE, "_pool_poison_child.py"), *args], env=env,
                       capture_output=True, text=True, timeout=150)
    print(f"\n_pool_poison_child {' '.join(args)} {env_extra}: {time.perf_counter() - t0:.1f} s")
    last = [ln for ln in r.stderr.splitlines() if ln.startswith("case ")][-1:]
    assert r.returncode == 0, (args, env_extra, f"exit {r.returncode}", "last case:", last, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def b_alone(gpu, tmp_path_factory):
    """B alone with the pool left alone, and the parts the oracle is compared with"""
    parts = str(tmp_path_factory.mktemp("pool_poison") / "parts.npz")
    out = _run(["--order", "b", "--parts", parts], {})
    return out, dict(np.load(parts))


@pytest.fixture(scope="module")
def baseline(gpu):
    return _run(["--order", "ab"], {})


def test_b_after_a_is_b_alone(b_alone, baseline):
    assert set(baseline) == set(K.CASES) and len(K.CASES) == 30
    differ = sorted(k for k in K.CASES if baseline[k] != b_alone[0].get(k))
    assert not differ, f"B after A differs from B alone in {differ}"


def _bytes(a):
    return np.asarray(a).tobytes()


def _transcript(O, root):
    t = O.Transcript(b"pool poison")
    t.append_message(b"polycommit", root)
    return t


def _check_proof(O, parts, case, o_enc, coeffs, field, seed, n_per_row):
    o_comm = O.Commit(o_enc, np.asarray(coeffs).reshape(-1))
    root = o_comm.root()
    assert _bytes(parts[f"{case}/root"]) == root, case
    outer = K.L.field_random(field, o_comm.n_rows, seed + 1)
    inner = K.L.field_random(field, n_per_row, seed + 2)
    pf = o_comm.prove(o_enc, outer.reshape(-1), _transcript(O, root))
    assert np.array_equal(parts[f"{case}/p_eval"].reshape(-1), pf.p_eval), case
    assert np.array_equal(parts[f"{case}/p_random"].reshape(-1), pf.p_random), case
    rc, ev = pf.verify(root, outer.reshape(-1), inner.reshape(-1), o_enc, _transcript(O, root))
    assert rc == 0 and np.array_equal(parts[f"{case}/ev"].reshape(-1), ev), case
    return root


def test_default_results_are_the_oracles(b_alone, gpu, oracle):
    """B's results with the pool left alone against the CPU oracle, for every case that has a counterpart
    there; the other cases are anchored by the child's own assertions"""
    O, (_, parts) = oracle, b_alone
    roots = {}
    for field in range(5):
        enc = gpu.LigeroEncoding.new(field, K.LIGERO_LEN)
        o_enc = O.Encoding.ligero(field, enc.n_per_row, enc.n_cols, enc.get_n_col_opens(), enc.get_n_degree_tests())
        roots[field] = _check_proof(O, parts, f"ligero_f{field}", o_enc, K.ligero_coeffs("B", field), field,
                                    K.seed_of("B", 20 + field), enc.n_per_row)
    assert _bytes(parts["ligero_device_f1/root"]) == roots[1]
    _check_proof(O, parts, "ligero_fused_f1", O.Encoding.ligero(1, K.FUSED_DIMS[0], K.FUSED_DIMS[1], 24, 2),
                 K.fused_coeffs("B"), 1, K.seed_of("B", 27), K.FUSED_DIMS[0])
    for field in (0, 1):
        enc = gpu.SdigEncoding.new(field, K.SDIG_LEN, 5, 3)
        _check_proof(O, parts, f"sdig_f{field}", O.Encoding.sdig(field, enc.n_per_row, seed=5, code_id=3),
                     K.sdig_coeffs("B", field), field, K.seed_of("B", 35 + field), enc.n_per_row)
    # the batch proofs' row combinations
    for field in (0, 1):
        enc = gpu.LigeroEncoding.new(field, 1 << K.BATCH_LG)
        coeffs = K.batch_coeffs("B", field)
        o_enc = O.Encoding.ligero(field, enc.n_per_row, enc.n_cols, enc.get_n_col_opens(), enc.get_n_degree_tests())
        o_comm = O.Commit(o_enc, coeffs.reshape(-1))
        assert _bytes(parts[f"batch_f{field}/root"]) == o_comm.root()
        for j, outer in enumerate(K.batch_outers("B", field, o_comm.n_rows)):
            want = O.collapse(field, coeffs.reshape(-1), outer.reshape(-1), o_comm.n_rows, o_comm.n_per_row)
            assert np.array_equal(parts[f"batch_f{field}/p_evals"][j].reshape(-1), want.reshape(-1)), (field, j)
    for k, (field, rows, cols) in enumerate(K.HASH_SHAPES):
        assert _bytes(parts[f"hash_columns/hash_{k}"]) == O.hash_columns(field, K.hash_matrix("B", k).reshape(-1), rows, cols), k
    leaves = K.merkle_leaves("B")
    level, tree = [leaves[i:i + 32] for i in range(0, len(leaves), 32)], []
    while len(level) > 1:
        level = [O.blake3(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
        tree += level
    assert _bytes(parts["merkle_tree/tree"]) == b"".join(tree)
    for j, (data, pre, enc, rows) in enumerate(K.fleet("B")):
        cap = 2 * rows + 3
        o_img, o_tree, o_rows, _ = O.pos_encode_file(data.tobytes(), pre, enc, cap)
        assert o_rows == rows and _bytes(parts[f"group_ingest/tree_{j}"]) == o_tree, j
        got = parts[f"group_ingest/img_{j}"].view("<u8").reshape(enc, cap)
        assert np.array_equal(got[:, :rows], np.frombuffer(o_img, "<u8").reshape(enc, cap)[:, :rows]), j
        assert (got[:, rows:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), j      # rows past rows_written: untouched


@pytest.mark.parametrize("poison", [0x00, 0xff, 0xa5], ids=["0x00", "0xff", "0xa5"])
def test_poisoned_blocks_give_the_same_results(baseline, poison):
    """0x00 is what fresh memory usually is, 0xff makes every unwritten element non-canonical and every
    unwritten flag set, 0xa5 is neither"""
    got = _run(["--order", "ab"], {"LCPC_POOL_POISON": str(poison)})
    differ = sorted(k for k in K.CASES if got.get(k) != baseline[k])
    assert not differ, f"LCPC_POOL_POISON={poison:#x} changes {differ}"


def test_the_switch_is_seen_to_act(gpu):
    """lcpc_selftest_pool_poison in a child of its own: 256, 4096 and 2^20 + 1 bytes, with and without a
    stream, a fresh block and then the recycled one (released holding the poison's complement)"""
    on = _run(["--probe"], {"LCPC_POOL_POISON": "165"})
    assert len(on) == 12 and {(r["bytes"], r["with_stream"]) for r in on} == \
        {(n, s) for n in (256, 4096, (1 << 20) + 1) for s in (True, False)}
    for r in on:
        assert r["enabled"] is True and (r["first"], r["last"]) == (0xa5, 0xa5), r
    off = _run(["--probe"], {})
    assert len(off) == 12 and not any(r["enabled"] for r in off)
