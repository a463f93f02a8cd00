"""The host-only verifier of the ext_log = 1 format (transcript.hpp, ProofFormat::ext) and the arithmetic of E (ext.hpp) compiled with
g++ -fsanitize=address,undefined as a stand-alone program (tests/ext_sanitizer_check.cpp) and run on model proofs of tests/ext_ref.py: valid,
truncated, bit-flipped, with huge path counts, read as the other ext_log, and random bytes.  CPU only; nothing is loaded into Python."""
import os
import subprocess

import pytest

import ext_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "ext_sanitizer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "ext_sanitizer_check.cpp"),
                           os.path.join(ROOT, "zkstark_amd", "csrc", "host_sha.cpp"), "-o", exe])
    return exe


# (log_n, log_b, K, coset, D, c, q, hash, grind): one-value leaves with the free term; 16-word coset leaves (a padding block, a chain of two
# field compressions) with a final polynomial; caps and grinding
@pytest.mark.parametrize("s", [(4, 1, 1, False, 0, 0, 1, 0, 0), (5, 2, 3, True, 2, 3, 3, 1, 0), (4, 2, 2, False, 0, 2, 2, 1, 4)],
                         ids=lambda s: "-".join(str(int(v)) for v in s))
def test_ext_verifier_memory_safety(orc, checker, tmp_path, s):
    log_n, log_b, K, coset, D, c, q, h, g = s
    ref = ext_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, g)
    (tmp_path / "proof.bin").write_bytes(ref.data)
    out = subprocess.run([checker, str(tmp_path / "proof.bin"), str(ref.public_last)] +
                         [str(int(v)) for v in (log_n, log_b, h, q, g, K, coset, D, c)] + [bytes(ref.state).hex()],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "field self-check: ok" in out.stdout and "format self-check" in out.stdout and "ok: valid accepted" in out.stdout
