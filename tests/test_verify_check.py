"""zk_verify_check (no GPU): the check number of the CPU verifier, the yardstick of the batched GPU verifier
(tests/test_gpu_verify_batch.py).  For every proof of the tamper corpus (tests/verify_corpus.py) it returns the number
zk_verify_queries names in zk_last_error, and agrees with it on accept or reject."""
import ctypes as C
import re

import pytest

import verify_corpus

SIZES = [(2, 1), (5, 2), (10, 3)]


def _queries_check(lib, it, log_n, log_b, q, hash_kind, strict):
    """(return code, check number named in zk_last_error) of zk_verify_queries."""
    rc = lib.zk_verify_queries(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q)
    if rc == 0:
        return rc, 0
    m = re.search(r"at check (-?\d+)", lib.zk_last_error().decode())
    assert m, lib.zk_last_error()
    return rc, int(m.group(1))


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("log_n,log_b", SIZES)
def test_check_number_matches_zk_verify_queries(zk, orc, log_n, log_b, q, hash_kind):
    lib = zk.load()
    items = verify_corpus.corpus(orc, log_n, log_b, q, hash_kind)
    assert len(items) > 60
    seen = set()
    for strict in (False, True):
        for it in items:
            out = C.c_int32(12345)
            rc = lib.zk_verify_check(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q,
                                     C.byref(out))
            want_rc, want_check = _queries_check(lib, it, log_n, log_b, q, hash_kind, strict)
            assert (rc, out.value) == (want_rc, want_check), (it.label, strict)
            seen.add(out.value)
    # the corpus reaches the transcript checks, the algebra, the paths and the malformed-layout numbers
    assert 0 in seen and -2 in seen and -1999 in seen and any(c <= -1000 for c in seen if c != -1999)
    assert any(-200 < c <= -100 for c in seen) and any(-500 < c <= -300 for c in seen)
    assert -1 in seen or -3 in seen or any(-300 < c <= -200 for c in seen)


def test_valid_proofs_pass_and_accepted_tampering_is_harmless(zk, orc):
    """Proof.check is the same number.  A variant the CPU accepts is one the checks cannot tell apart from the proof: a raw
    challenge plus P (used reduced; the strict replay sees it), a wrong state or a changed root of the last layer (only the
    strict replay reads them: verify_proof checks the paths of layers 0 .. R-1), or public_last plus P (used reduced, and not
    part of the transcript)."""
    items = verify_corpus.corpus(orc, 5, 2, 1, 0)
    for it in items:
        p = zk.Proof(it.state, it.data, 5, 2, it.public_last)
        plain, strict = p.check(), p.check(strict=True)
        if it.label.endswith(".valid"):
            assert plain == 0 and strict == 0
        if plain == 0 and not it.label.endswith(".valid"):
            assert re.search(r"\.(alpha\d|beta\d+)\.plusP$|\.state$|public_last\+P$|\.layer_root4\.\w+$", it.label), it.label
        if strict == 0 and not it.label.endswith(".valid"):
            assert it.label.endswith("public_last+P"), it.label


def test_argument_errors(zk, orc):
    lib = zk.load()
    (data, state, last), _ = verify_corpus.oracle_proofs(orc, 5, 2, 1, 0)
    out = C.c_int32(777)
    assert lib.zk_verify_check(None, len(data), None, 5, 2, last, 0, 1, C.byref(out)) == -1 and out.value == 777
    assert lib.zk_verify_check(data, len(data), None, 5, 2, last, 2, 1, C.byref(out)) == -1 and out.value == 777
    assert lib.zk_verify_check(data, len(data), None, 5, 2, last, 0, 1, None) == -1
    assert lib.zk_verify_check(data, len(data), state, 5, 2, last, 0, 1, C.byref(out)) == 0 and out.value == 0
    # unsupported sizes, query counts and lengths are rejected proofs (-1), exactly as zk_verify_queries treats them
    for args in ((1, 2, 1), (5, 0, 1), (5, 2, 0), (5, 2, 65)):
        assert lib.zk_verify_check(data, len(data), None, *args[:2], last, 0, args[2], C.byref(out)) == -6 and out.value == -1
    assert lib.zk_verify_check(data, len(data) - 4, None, 5, 2, last, 0, 1, C.byref(out)) == -6 and out.value == -1
    assert lib.zk_verify_check(data + bytes(4), len(data) + 4, None, 5, 2, last, 0, 1, C.byref(out)) == -6 and out.value == -8
