"""The product's host-only code (transcript.hpp: channel, wire format, verifier; fieldhash.hpp on the
host) compiled with g++ -fsanitize=address,undefined and run on valid, truncated, bit-flipped and random
proofs.  CPU only (GPU sanitizers are not available on the pool)."""
import os
import platform
import subprocess

import pytest

import cap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_argv(exe, san):
    """The command that runs a checker built with -fsanitize=`san`.  The ThreadSanitizer runtime of older GCCs (11 among them)
    expects the address layout of a kernel that randomises mmap with at most 28 bits: on a kernel that uses more it stops before
    main ("FATAL: ThreadSanitizer: unexpected memory mapping").  So the TSan build runs with address randomisation switched off
    for that one process (setarch -R, the child's own personality); what it checks is unchanged."""
    return ["setarch", platform.machine(), "-R", exe] if "thread" in san else [exe]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "host_sanitizer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "host_sanitizer_check.cpp"),
                           os.path.join(ROOT, "zkstark_amd", "csrc", "host_sha.cpp"), "-o", exe])
    return exe


# settings: None = the reference's format through the lax verifier alone; (q, K, coset, D, c, grind) = that format (tests/cap_ref.py builds
# the proof) through the replay and then the proof checks, with the proof's state.  The checker also walks ProofFormat's own grid.
@pytest.mark.parametrize("log_n,log_b,hash_kind,settings", [
    pytest.param(6, 2, 0, None, id="6-2-0"), pytest.param(10, 3, 0, None, id="10-3-0"), pytest.param(5, 1, 1, None, id="5-1-1"),
    pytest.param(6, 3, 0, (3, 3, True, 2, 2, 4), id="every-setting")])
def test_verifier_memory_safety(orc, checker, tmp_path, log_n, log_b, hash_kind, settings):
    extra = []
    if settings is None:
        try:
            orc.set_hash(hash_kind)
            r = orc.prove(log_n, log_b, want_vectors=False)
        finally:
            orc.set_hash(0)
        assert r.rc == 0
        data, public_last = r.proof, r.public_last
    else:
        q, K, coset, D, c, grind = settings
        ref = cap_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits=grind)
        data, public_last = ref.data, ref.public_last
        extra = [str(q), str(grind), str(K), str(int(coset)), str(D), str(c), bytes(ref.state).hex()]
    p = tmp_path / "proof.bin"
    p.write_bytes(data)
    out = subprocess.run([checker, str(p), str(log_n), str(log_b), str(public_last), str(hash_kind)] + extra,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "format self-check" in out.stdout and "ok: valid accepted" in out.stdout


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_batch_pool_under_sanitizers(tmp_path, san):
    """The fork-join pool of the batched prover (csrc/pool.hpp): lock-free job hand-off with spinning and blocking
    workers, run under ThreadSanitizer and ASan/UBSan."""
    exe = str(tmp_path / "pool_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={san}", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pool_check.cpp"), "-o", exe])
    out = subprocess.run(_run_argv(exe, san), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pool ok" in out.stdout


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_root_board_under_sanitizers(tmp_path, san):
    """The shared-memory exchange of subtree roots between the ranks of the sharded prover (csrc/board.hpp):
    1-8 ranks, thousands of exchanges with skewed timing, size mismatch, a dead rank (timeout)."""
    exe = str(tmp_path / "board_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={san}", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "board_check.cpp"), "-o", exe, "-lrt"])
    out = subprocess.run(_run_argv(exe, san), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "board ok" in out.stdout


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_peer_copy_protocol_under_sanitizers(tmp_path, san):
    """The peer-copy transport of the sharded prover (csrc/peer.hpp, round 6) with host memory standing in for the GPU (the device
    runtime is a policy of the transport; -DZK_PEER_NO_HIP): 1-8 ranks as threads, thousands of all-to-alls and all-gathers of
    changing sizes with skewed timing and every word checked, a collective larger than the staging buffer, a rank that leaves
    (its peers return at once, naming it), a rank that never comes (bounded; nothing left in /dev/shm).  Under ThreadSanitizer the
    release / acquire pairs on the shared page are mirrored on process-wide keys (every rank maps the page at its own address);
    dropping the second meeting of a collective makes this test fail with data races (checked by hand in round 6)."""
    exe = str(tmp_path / "peer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={san}", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "peer_check.cpp"), "-o", exe, "-lrt"])
    out = subprocess.run(_run_argv(exe, san), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr[-4000:]
    assert "peer transport protocol ok" in out.stdout
