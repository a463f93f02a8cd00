"""The host-only verifier with row leaves (transcript.hpp, ProofFormat::rows) and the row leaf hash compiled with
g++ -fsanitize=address,undefined as a stand-alone program (tests/rows_sanitizer_check.cpp) and run on a model proof of tests/rows_ref.py:
valid, truncated, bit-flipped, with huge path counts, read without row leaves and as another width, and random bytes; the leaf hash at
every width from buffers of exactly that many values.  CPU only; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import rows_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("san") / "rows_sanitizer_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "rows_sanitizer_check.cpp"),
                           os.path.join(ROOT, "zkstark_amd", "csrc", "host_sha.cpp"), "-o", exe])
    return exe


# (log_n, log_b, lb, K, coset, D, c, q, hash, grind): one compression per row; a chain of two field compressions; 256 values per row
@pytest.mark.parametrize("s", [(4, 1, 1, 1, False, 0, 0, 1, 0, 0), (5, 2, 3, 3, True, 2, 3, 3, 1, 0), (4, 2, 4, 2, False, 0, 2, 2, 1, 4),
                               (4, 1, 8, 1, True, 0, 1, 2, 0, 0)],
                         ids=lambda s: "-".join(str(int(v)) for v in s))
def test_rows_verifier_memory_safety(orc, checker, tmp_path, s):
    log_n, log_b, lb, K, coset, D, c, q, h, g = s
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, g)
    (tmp_path / "proof.bin").write_bytes(ref.data)
    (tmp_path / "last.bin").write_bytes(np.array(ref.public_last, dtype="<u4").tobytes())
    out = subprocess.run([checker, str(tmp_path / "proof.bin"), str(tmp_path / "last.bin")] +
                         [str(int(v)) for v in (log_n, log_b, lb, h, q, g, K, coset, D, c)] + [bytes(ref.state).hex()],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "format self-check" in out.stdout and "leaf self-check" in out.stdout and "ok: valid accepted" in out.stdout
