"""CPU: the work lists of the grouped ingest, scrub and repair planners against
tests/golden/pos_group_plans.json, recorded before the three planners became one.  Every record of
every fleet of tests/golden/gen_pos_group_plans.py is recomputed -- at the default group size and with
LCPC_POS_GROUP_BYTES lowered to 65536 and to 4096 -- and compared: tile count, launch count and the
SHA-256 of the tile array's bytes.  The other plan tests check what a work list promises; this one
that not one tile moved."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_gen():
    spec = importlib.util.spec_from_file_location("gen_pos_group_plans", os.path.join(GOLDEN, "gen_pos_group_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_gen()
FLEETS = GEN.fleets()
with open(os.path.join(GOLDEN, "pos_group_plans.json")) as _fh:
    RECORDED = json.load(_fh)


@pytest.fixture(scope="module")
def pos():
    from lcpc_proof_of_storage_amd import pos as P
    return P


def test_the_golden_covers_the_fleets_and_stays_small():
    assert sorted(RECORDED) == sorted(FLEETS)
    assert os.path.getsize(os.path.join(GOLDEN, "pos_group_plans.json")) < 64 << 10
    for name, f in FLEETS.items():
        rec = RECORDED[name]
        assert rec["n_jobs"] == len(f["enc"]) and rec["seed"] == f["seed"]
        assert rec["fleet_sha256"] == GEN.fleet_sha(f), name       # the fleet is the one that was recorded
        assert sorted(rec["plans"]) == sorted(GEN.group_bytes_key(gb) for gb in GEN.GROUP_BYTES)


def test_the_fleets_hold_what_they_are_for():
    f = FLEETS["every_enc_pre_rows"]
    assert set(f["enc"]) == set(1 << k for k in range(1, 12))
    assert set(f["rows"]) == {0, 1, 7, 8, 9, 124, 125, 1023, 1024, 1025}
    jobs = set(zip(f["enc"], f["pre"]))
    for enc in set(f["enc"]):
        assert (enc, 1) in jobs and (enc, enc - 1) in jobs
        assert enc < 4 or any(e == enc and p & (p - 1) for e, p in jobs)
    kinds = {(b == 0, b == 1, b == e - p, b == e - p + 1) for e, p, b in zip(f["enc"], f["pre"], f["n_bad"])}
    assert len(kinds) >= 4
    assert len(FLEETS["one_row_jobs"]["enc"]) > GEN.MAX_JOBS
    g = FLEETS["repair_no_work_only"]
    assert all(b == e - p + 1 for e, p, b in zip(g["enc"], g["pre"], g["n_bad"]))


@pytest.mark.parametrize("group_bytes", GEN.GROUP_BYTES, ids=GEN.group_bytes_key)
@pytest.mark.parametrize("name", sorted(FLEETS))
def test_every_plan_is_the_recorded_one(pos, monkeypatch, name, group_bytes):
    if group_bytes is None:
        monkeypatch.delenv("LCPC_POS_GROUP_BYTES", raising=False)
    else:
        monkeypatch.setenv("LCPC_POS_GROUP_BYTES", str(group_bytes))
    got = GEN.records(pos, FLEETS[name])
    want = RECORDED[name]["plans"][GEN.group_bytes_key(group_bytes)]
    for entry in ("ingest_plan", "scrub_plan", "repair_plan"):
        assert got[entry] == want[entry], (name, group_bytes, entry)
