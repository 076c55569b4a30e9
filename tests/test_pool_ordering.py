"""The stream-ordered device pool (lcpc_proof_of_storage_amd/csrc/pool.hpp) on a simulated device
(CPU, no HIP): a block's next owner is ordered after every use still queued on any stream that
used it, under 200 random interleavings plus the directed cases (own stream: no wait; completed
fence: free; host taker: host wait; events reused only after their record completed).
tests/cpp/test_pool.cpp, built with ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pool_ordering_on_simulated_streams(tmp_path):
    exe = tmp_path / "test_pool"
    src = os.path.join(ROOT, "tests", "cpp", "test_pool.cpp")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-o", str(exe), src], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pool ordering: ok" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pool_ordering_from_many_threads(tmp_path):
    """The same property with 8 host threads on one pool (take / put / order_after under its mutex,
    the backend called outside it) while a simulated device thread retires the streams' operations
    in random order: tests/cpp/test_pool_threads.cpp, built with ThreadSanitizer.  No block may be
    owned twice, no earlier owner's write may complete after a later owner's first read, and the
    pool's own state must be free of data races."""
    exe = tmp_path / "test_pool_threads"
    src = os.path.join(ROOT, "tests", "cpp", "test_pool_threads.cpp")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=thread", "-Wall", "-o", str(exe), src],
                   check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pool threads: ok" in r.stdout
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.gpu
def test_pool_ordering_on_device():
    """The same fences on the MI355X (lcpc_selftest_pool_ordering): a block released while a
    late writer (spinning 300 us) still owns it is taken on another stream and overwritten at
    once; no word may read the late writer's value.  The unfenced control round shows the test
    can see a violation when the streams run concurrently (reported, not asserted: two streams
    may share a hardware queue)."""
    import lcpc_proof_of_storage_amd as L
    L.set_device(0)
    r = L.selftest_pool_ordering(rounds=8, spin_us=300)
    print("pool selftest:", r)
    assert r["violations"] == 0, r
    assert r["reused"] >= 16, r  # the fenced rounds took back the released block
