"""Proof-of-work grinding without a GPU (DESIGN.md "Grinding"): the host search against a hashlib scan, the proof length, and the
CPU verifiers (zk_verify_grind, Proof.check / verify) on grinding proofs built without the library (tests/grind_ref.py)."""
import ctypes as C
import random
import struct

import pytest

import grind_ref

P = 3221225473


def test_reference_builder_is_the_oracle_at_g0(orc):
    """grind_ref with g = 0 reproduces the oracle's own proof, so its decommitment assembly is the prover's."""
    for log_n, log_b, q, h in ((5, 2, 1, 0), (4, 1, 7, 1)):
        data, state, last, _ = grind_ref.grind_proof(orc, log_n, log_b, q, h, 0)
        orc.set_queries(q)
        orc.set_hash(h)
        try:
            r = orc.prove(log_n, log_b, 1, 3141592, want_vectors=False)
        finally:
            orc.set_queries(1)
            orc.set_hash(0)
        assert (data, state, last) == (r.proof, r.state, r.public_last)


def test_host_search_equals_a_hashlib_scan(zk):
    lib = zk.load()
    rng = random.Random(20)
    for g in range(1, 15):
        for i in range(50):
            st = bytes(rng.getrandbits(8) for _ in range(32))
            start = (0, 2**32 - 3, 2**33 - 1, rng.getrandbits(36))[i % 4]
            want = grind_ref.smallest_nonce(st, g, start)
            out = C.c_uint64(7)
            assert lib.zk_grind_host(st, g, start, (1, 3, 16)[i % 3], C.byref(out)) == 0
            assert out.value == want, (g, i, start)
    st = bytes(range(32))
    assert zk.grind_host(st, 0, 12345) == 12345                      # g = 0: the start itself
    assert zk.grind_host(st, 10) == grind_ref.smallest_nonce(st, 10)


def test_argument_errors(zk):
    lib = zk.load()
    out = C.c_uint64(7)
    assert lib.zk_grind_host(bytes(32), 33, 0, 1, C.byref(out)) == -1 and out.value == 7
    assert lib.zk_grind_host(None, 4, 0, 1, C.byref(out)) == -1
    assert lib.zk_grind_host(bytes(32), 4, 2**64 - 5, 1, C.byref(out)) == -1   # start + 2^44 overflows
    # the setters take no handle on a machine without a GPU: a null one is refused before the range check
    assert lib.zk_ctx_set_grinding(None, 4) == -1 and lib.zk_verifier_set_grinding(None, 4) == -1
    assert lib.zk_batch_set_grinding(None, 4) == -1


def test_proof_length(zk):
    lib = zk.load()
    for log_n, log_b, q in ((2, 1, 1), (10, 3, 1), (5, 2, 7), (21, 3, 64)):
        base = lib.zk_proof_data_len_queries(log_n, log_b, q)
        assert lib.zk_proof_data_len_grind(log_n, log_b, q, 0) == base
        for g in (1, 16, 32):
            assert lib.zk_proof_data_len_grind(log_n, log_b, q, g) == base + 8


def _check(lib, data, state, log_n, log_b, last, h, q, g):
    out = C.c_int32(12345)
    rc = lib.zk_verify_grind(data, len(data), state, log_n, log_b, last, h, q, g, C.byref(out))
    assert rc == (0 if out.value == 0 else -6)
    return out.value


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b", [(2, 1), (5, 2), (10, 3)])
def test_cpu_verifiers_accept_grinding_proofs(zk, orc, log_n, log_b, hash_kind):
    lib = zk.load()
    name = ("sha256", "field")[hash_kind]
    for q in (1, 3):
        for g in (1, 8):
            data, state, last, w = grind_ref.grind_proof(orc, log_n, log_b, q, hash_kind, g)
            assert len(data) == lib.zk_proof_data_len_grind(log_n, log_b, q, g)
            assert _check(lib, data, state, log_n, log_b, last, hash_kind, q, g) == 0
            assert _check(lib, data, None, log_n, log_b, last, hash_kind, q, g) == 0
            p = zk.Proof(state, data, log_n, log_b, last, name, q, grind_bits=g)
            assert p.check(strict=True) == 0 and p.check() == 0
            p.verify(strict=True)
            p.verify()


@pytest.mark.parametrize("log_n,log_b,q", [(5, 2, 1), (4, 3, 3)])
def test_nonce_tampering(zk, orc, log_n, log_b, q):
    lib = zk.load()
    g = 6
    data, state, last, w = grind_ref.grind_proof(orc, log_n, log_b, q, 0, g)
    off = grind_ref.prefix_len(log_n)
    assert struct.unpack("<Q", data[off:off + 8])[0] == w
    s = grind_ref.replay_prefix(data, log_n)
    # a nonce that misses the bits: -1998 when strict (before any query challenge), accepted when not (the work is not checked there)
    bad = next(v for v in range(w + 1, w + 10**6) if not grind_ref.meets(s, g, v))
    forged = data[:off] + struct.pack("<Q", bad) + data[off + 8:]
    assert _check(lib, forged, state, log_n, log_b, last, 0, q, g) == -1998
    assert _check(lib, forged, None, log_n, log_b, last, 0, q, g) == 0
    assert zk.Proof(state, forged, log_n, log_b, last, queries=q, grind_bits=g).check(strict=True) == -1998
    with pytest.raises(zk.ZkError):
        zk.Proof(state, forged, log_n, log_b, last, queries=q, grind_bits=g).verify(strict=True)
    # the NEXT valid nonce passes the bits but moves the transcript: the first query challenge is then wrong
    nxt = grind_ref.smallest_nonce(s, g, w + 1)
    forged = data[:off] + struct.pack("<Q", nxt) + data[off + 8:]
    assert _check(lib, forged, state, log_n, log_b, last, 0, q, g) == -(1000 + 3 + log_n + 1)
    assert _check(lib, forged, None, log_n, log_b, last, 0, q, g) == 0
    # the whole proof with that nonce is as valid as the prover's: the verifier accepts any nonce that meets the bits
    other, ost, olast, _ = grind_ref.grind_proof(orc, log_n, log_b, q, 0, g, nonce=nxt)
    assert _check(lib, other, ost, log_n, log_b, olast, 0, q, g) == 0


def test_length_must_match_the_grinding(zk, orc):
    lib = zk.load()
    data, state, last, _ = grind_ref.grind_proof(orc, 5, 2, 1, 0, 4)
    plain, pstate, plast, _ = grind_ref.grind_proof(orc, 5, 2, 1, 0, 0)
    assert _check(lib, data, state, 5, 2, last, 0, 1, 0) == -1            # a g > 0 proof read as g = 0
    assert _check(lib, data, None, 5, 2, last, 0, 1, 0) != 0
    assert _check(lib, plain, pstate, 5, 2, plast, 0, 1, 4) == -1         # a g = 0 proof read as g > 0
    assert _check(lib, plain, None, 5, 2, plast, 0, 1, 4) == -1
    assert _check(lib, data, state, 5, 2, last, 0, 1, 33) == -1           # g > 32 is no proof size
    assert _check(lib, plain, pstate, 5, 2, plast, 0, 1, 0) == 0
