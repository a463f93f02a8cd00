"""Early stop of FRI without a GPU (zk_verify_stop, zk_proof_data_len_stop; DESIGN.md 7d "Early stop"): the proof length against
tests/stop_ref.py over every admissible stop_log, the CPU verifier against the plain-Python one -- accepted proofs and, for tampered
ones, the same check number -- the formats rejecting each other, and stop_log = 0 being zk_verify_fold / zk_verify_coset."""
import ctypes as C

import pytest

import coset_ref
import fold_ref
import stop_ref

SHAPES = [(4, 1), (5, 2), (6, 3)]


def _check(lib, data, state, log_n, log_b, last, h, q, g, K, coset, D):
    out = C.c_int32(12345)
    rc = lib.zk_verify_stop(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, int(coset), D, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value)
    return out.value


def _check_plain(lib, data, state, log_n, log_b, last, h, q, g, K, coset):
    out = C.c_int32(12345)
    fn = lib.zk_verify_coset if coset else lib.zk_verify_fold
    rc = fn(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value)
    return out.value


def _stops(log_n, log_b):
    return sorted(d for d in {1, 2, log_n - 1} if stop_ref.admissible(log_n, log_b, d))


def test_proof_length(zk):
    lib = zk.load()
    n = 0
    for log_n in (2, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        for log_b in (1, 2, 3, 4):
            for q in (1, 3):
                for g in (0, 5):
                    for K in (1, 2, 3):
                        for coset in (0, 1):
                            for D in range(0, 14):
                                got = lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, coset, D)
                                if stop_ref.admissible(log_n, log_b, D):
                                    assert got == stop_ref.proof_len(log_n, log_b, q, g, K, coset, D), (log_n, log_b, q, g, K, coset, D)
                                    n += D > 0
                                else:
                                    assert got == 0, (log_n, log_b, q, g, K, coset, D)
                            plain = lib.zk_proof_data_len_coset if coset else lib.zk_proof_data_len_fold
                            assert lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, coset, 0) == plain(log_n, log_b, q, g, K)
    assert n > 1000
    # outside the limits: D = log_n, D = 9, D + log_b = 13, a bad fold_log
    assert lib.zk_proof_data_len_stop(6, 3, 1, 0, 1, 0, 6) == 0 and lib.zk_proof_data_len_stop(6, 3, 1, 0, 1, 0, 5) != 0
    assert lib.zk_proof_data_len_stop(12, 3, 1, 0, 1, 0, 9) == 0 and lib.zk_proof_data_len_stop(12, 3, 1, 0, 1, 0, 8) != 0
    assert lib.zk_proof_data_len_stop(12, 5, 1, 0, 1, 0, 8) == 0 and lib.zk_proof_data_len_stop(12, 5, 1, 0, 1, 0, 7) != 0
    assert lib.zk_proof_data_len_stop(10, 3, 1, 0, 0, 0, 2) == 0 and lib.zk_proof_data_len_stop(10, 3, 1, 0, 4, 1, 2) == 0
    # a stopped proof is shorter: every dropped group's tuples and 36 header bytes go, 4 * 2^D - 4 bytes of coefficients come.
    # With coset leaves and K > 1 that holds when whole groups are dropped (D a multiple of K): a SHORTER last group is a leaf of
    # fewer slots under a longer path, which can cost more than it saves (K = 3, D = 1 at 2^24: 170 800 bytes against 170 316).
    for coset in (0, 1):
        for K in (1, 2, 3):
            full = lib.zk_proof_data_len_stop(21, 3, 32, 0, K, coset, 0)
            assert all(lib.zk_proof_data_len_stop(21, 3, 32, 0, K, coset, D) < full for D in range(1, 9) if not coset or D % K == 0)
    assert [lib.zk_proof_data_len_stop(21, 3, 32, 0, 3, 1, D) for D in (0, 1, 3, 6)] == [170316, 170800, 165924, 158688]
    assert [lib.zk_proof_data_len_stop(21, 3, 32, 0, 1, 0, D) for D in (0, 4, 8)] == [719044, 670800, 590720]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_cpu_verifier_accepts_reference_proofs(zk, orc, K, coset, hash_kind):
    lib = zk.load()
    i = 0
    for log_n, log_b in SHAPES:
        for D in _stops(log_n, log_b):
            q, g = ((1, 0), (3, 5), (1, 5), (3, 0))[i % 4]
            i += 1
            ref = stop_ref.stop_proof(orc, log_n, log_b, q, hash_kind, K, coset, D, g)
            assert len(ref.data) == lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, int(coset), D)
            assert len(ref.coef) == 1 << D
            args = (log_n, log_b, ref.public_last, hash_kind, q, g, K, coset, D)
            assert stop_ref.verify(orc, ref.data, ref.state, *args) == 0, args
            assert stop_ref.verify(orc, ref.data, None, *args) == 0, args
            assert _check(lib, ref.data, ref.state, *args) == 0, args
            assert _check(lib, ref.data, None, *args) == 0, args


def _tampered(data, regs):
    """(name, bytes): one flipped byte per region, one byte less, one byte more, and the last path one digest shorter."""
    for name, off, n in regs:
        pos = off + (n // 2 if n > 8 else 0)                # a u64 count: its low byte; a digest / path: a byte in the middle
        bad = bytearray(data)
        bad[pos] ^= 0x01 if ".count" in name else 0x40
        yield name, bytes(bad)
    name, off, n = [r for r in regs if ".count" in r[0]][-1]
    bad = bytearray(data)
    bad[off] -= 1
    yield "last count - 1", bytes(bad)
    yield "truncated", data[:-1]
    yield "appended", data + b"\0"


@pytest.mark.parametrize("log_n,log_b,K,coset,D,q,g,hash_kind", [
    (5, 2, 2, False, 2, 2, 0, 0),                           # R' = 3: groups of 2 + 1
    (6, 3, 3, True, 1, 1, 5, 1),                            # R' = 5: groups of 3 + 2, coset leaves, field hash, grinding
    (4, 1, 1, False, 3, 1, 5, 1),                           # R' = 1: a single group of one step
    (6, 3, 1, True, 5, 2, 0, 0),                            # 32 coefficients, one coset group
    (6, 3, 2, False, 2, 1, 0, 0),
])
def test_tampered_proofs_get_the_same_check_number(zk, orc, log_n, log_b, K, coset, D, q, g, hash_kind):
    lib = zk.load()
    ref = stop_ref.stop_proof(orc, log_n, log_b, q, hash_kind, K, coset, D, g)
    args = (log_n, log_b, ref.public_last, hash_kind, q, g, K, coset, D)
    regs = stop_ref.regions(log_n, log_b, q, g, K, coset, D)
    G = len(fold_ref.groups(log_n - D, K))
    names = [r[0] for r in regs]
    assert all(f"coef{k}" in names for k in range(1 << D)) and f"beta{G - 1}" in names and f"root{G}" not in names
    assert any(nm.startswith(f"q0.g{G - 1}.") for nm in names)
    seen, by_name = set(), {}
    for name, bad in _tampered(ref.data, regs):
        for state in (ref.state, None):
            want = stop_ref.verify(orc, bad, state, *args)
            got = _check(lib, bad, state, *args)
            assert got == want, (name, state is not None, got, want)
            seen.add(got)
            by_name[(name, state is not None)] = got
            if state is not None or not name.startswith(("alpha", "beta", "raw", "nonce")):
                # lax mode reads challenges from the proof (as the reference does); a changed beta then fails the fold it feeds
                assert got != 0 or name == "nonce", (name, state is not None)
    # every coefficient is bound twice: by the transcript (strict) and by the last group's fold against p(x^(2^R')) (lax too)
    for k in range(1 << D):
        assert by_name[(f"coef{k}", False)] == -(100 + G - 1), k
        assert -1100 < by_name[(f"coef{k}", True)] <= -1000 or by_name[(f"coef{k}", True)] == -1998
    assert by_name[(f"beta{G - 1}", False)] == -(100 + G - 1)
    first = "slot0" if coset else "value0"
    assert by_name[(f"q0.g{G - 1}.{first}", False)] in (-(100 + G - 1), -(100 + G - 2), -2)
    assert by_name[("truncated", False)] == by_name[("appended", True)] == -1
    assert {-1, -2, -4, -5, -6, -(100 + G - 1), -(200 + G - 1), -(300 + G - 1)} <= seen, sorted(seen)


@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_other_formats_are_refused_by_length(zk, orc, K, coset):
    lib = zk.load()
    for log_n, log_b in ((5, 2), (6, 3)):
        full = stop_ref.stop_proof(orc, log_n, log_b, 1, 0, K, coset, 0)
        for D in (1, 2):
            ref = stop_ref.stop_proof(orc, log_n, log_b, 1, 0, K, coset, D)
            for strict in (True, False):
                for other in (D - 1, D + 1):                # D off by one (D - 1 = 0: the verifier of full proofs)
                    st = ref.state if strict else None
                    assert _check(lib, ref.data, st, log_n, log_b, ref.public_last, 0, 1, 0, K, coset, other) == -1, (D, other, strict)
                    assert stop_ref.verify(orc, ref.data, st, log_n, log_b, ref.public_last, 0, 1, 0, K, coset, other) == -1
                st = full.state if strict else None         # a plain proof given to D > 0
                assert _check(lib, full.data, st, log_n, log_b, full.public_last, 0, 1, 0, K, coset, D) == -1
                assert stop_ref.verify(orc, full.data, st, log_n, log_b, full.public_last, 0, 1, 0, K, coset, D) == -1
                st = ref.state if strict else None          # the other leaf format, and limits broken
                assert _check(lib, ref.data, st, log_n, log_b, ref.public_last, 0, 1, 0, K, not coset, D) == -1
                assert _check(lib, ref.data, st, log_n, log_b, ref.public_last, 0, 1, 0, K, coset, log_n) == -1
                assert _check(lib, ref.data, st, log_n, log_b, ref.public_last, 0, 1, 0, K, coset, 9) == -1


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
def test_stop_zero_is_the_full_verifier_on_a_tampered_corpus(zk, orc, coset, hash_kind):
    """stop_log = 0 goes through the same function as zk_verify_fold / zk_verify_coset: the same number for every input."""
    lib = zk.load()
    for log_n, log_b, K, q, g in ((5, 2, 2, 2, 0), (6, 3, 3, 1, 8), (4, 1, 1, 1, 0)):
        ref = (coset_ref.coset_proof if coset else fold_ref.fold_proof)(orc, log_n, log_b, q, hash_kind, K, g)
        args = (log_n, log_b, ref.public_last, hash_kind, q, g, K, coset)
        assert len(ref.data) == lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, int(coset), 0)
        corpus = [ref.data, ref.data[:-1], ref.data + b"\0", ref.data[:100]]
        for pos in range(0, len(ref.data), 11):
            bad = bytearray(ref.data)
            bad[pos] ^= 0x01 if pos % 3 else 0x40
            corpus.append(bytes(bad))
        seen = set()
        for bad in corpus:
            for state in (ref.state, None):
                want = _check_plain(lib, bad, state, *args)
                assert _check(lib, bad, state, *args, 0) == want
                seen.add(want)
        assert 0 in seen and len(seen) > 6, sorted(seen)
    out = C.c_int32()
    assert lib.zk_verify_stop(None, 0, None, 5, 2, 0, 0, 1, 0, 1, 0, 0, C.byref(out)) == -1      # ZK_ERR_INVALID: null proof
    assert lib.zk_verify_stop(b"x", 1, None, 5, 2, 0, 7, 1, 0, 1, 0, 0, C.byref(out)) == -1      # unknown hash
    assert lib.zk_verify_stop(b"x", 1, None, 5, 2, 0, 0, 1, 0, 4, 0, 0, C.byref(out)) == -1      # fold_log out of range


def test_python_proof_goes_through_the_stop_functions(zk, orc):
    ref = stop_ref.stop_proof(orc, 6, 3, 3, 1, 2, True, 2, 5)
    p = zk.Proof(ref.state, ref.data, 6, 3, ref.public_last, "field", 3, 5, 2, True, stop_log=2)
    assert p.data_len() == p.expected_len() == len(ref.data) == stop_ref.proof_len(6, 3, 3, 5, 2, True, 2)
    assert p.check() == 0 and p.check(strict=True) == 0
    p.verify()
    p.verify(strict=True)
    bad = zk.Proof(ref.state, ref.data, 6, 3, ref.public_last, "field", 3, 5, 2, True, stop_log=1)
    assert bad.check() == -1
    with pytest.raises(zk.ZkError):
        bad.verify()
    assert zk.Proof(ref.state, ref.data, 6, 3, ref.public_last, "field", 3, 5, 2, True).check(strict=True) == -1
    assert zk.load().zk_ctx_get_fri_stop(None) == 0
