"""FRI folding factor 2^K without a GPU (DESIGN.md "Folding factor"): the proofs tests/fold_ref.py builds from the oracle's
primitives, the identity that defines a group's output, the proof length, and the CPU verifier zk_verify_fold against the
plain-Python verifier of fold_ref -- accepted proofs and, for tampered ones, the same check number."""
import ctypes as C
import struct

import numpy as np
import pytest

import fold_ref
import verify_corpus

P = fold_ref.P


def _check(lib, data, state, log_n, log_b, last, h, q, g, K):
    out = C.c_int32(12345)
    rc = lib.zk_verify_fold(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value)
    return out.value


@pytest.mark.parametrize("log_n,log_b,q,h", [(4, 1, 1, 0), (5, 2, 3, 0), (7, 3, 1, 1), (10, 3, 1, 0)])
def test_reference_builder_is_the_oracle_at_k1(orc, log_n, log_b, q, h):
    """fold_ref with K = 1 reproduces oracle.prove byte for byte, so its transcript and decommitment assembly are the prover's."""
    ref = fold_ref.fold_proof(orc, log_n, log_b, q, h, 1)
    orc.set_queries(q)
    orc.set_hash(h)
    try:
        r = orc.prove(log_n, log_b, 1, 3141592, want_vectors=False)
    finally:
        orc.set_queries(1)
        orc.set_hash(0)
    assert (ref.data, ref.state, ref.public_last) == (r.proof, r.state, r.public_last)


@pytest.mark.parametrize("log_n,log_b", [(5, 2), (7, 3), (10, 3)])
def test_k_fold_identity_against_the_coefficient_form(orc, log_n, log_b):
    """`steps` reference folds with beta, beta^2, beta^4, ... equal f_0 + beta f_1 + ... + beta^(2^K - 1) f_(2^K - 1) of the
    coefficients split by index mod 2^K, re-evaluated on the coset (w^(2^K)) <h^(2^K)>."""
    L = log_n + log_b
    N = 1 << L
    rng = np.random.default_rng(log_n)
    h = orc.gen_of_order_log(L)
    for K in (1, 2, 3, 4):
        for beta_raw in (int(rng.integers(0, P)), 0, 1, P - 1, P + 12345, 2**32 - 1):
            coef = rng.integers(0, P, 1 << log_n, dtype=np.uint64).astype(np.uint32)
            # evaluations on w h^i: scale coefficient k by w^k, then a size-N transform of the zero-padded vector
            scaled = np.array([int(c) * pow(5, k, P) % P for k, c in enumerate(coef)] + [0] * (N - len(coef)), dtype=np.uint32)
            layer = orc.ntt(scaled, h)
            got = fold_ref.fold_layer(orc, layer, log_n, log_b, 0, K, beta_raw)
            b, S = beta_raw % P, 1 << K
            folded = [sum(int(coef[S * i + t]) * pow(b, t, P) for t in range(S)) % P for i in range(len(coef) // S)]
            w = pow(5, S, P)
            scaled = np.array([c * pow(w, k, P) % P for k, c in enumerate(folded)] + [0] * ((N >> K) - len(folded)), dtype=np.uint32)
            want = orc.ntt(scaled, pow(h, S, P))
            assert np.array_equal(got, want), (K, beta_raw)


def test_proof_length(zk, orc):
    lib = zk.load()
    for log_n in (2, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        for log_b in (1, 2, 3, 4):
            for q in (1, 7):
                for g in (0, 12):
                    assert lib.zk_proof_data_len_fold(log_n, log_b, q, g, 1) == lib.zk_proof_data_len_grind(log_n, log_b, q, g)
                    for K in (1, 2, 3):
                        assert lib.zk_proof_data_len_fold(log_n, log_b, q, g, K) == fold_ref.proof_len(log_n, log_b, q, g, K)
    for K in (1, 2, 3):                                     # ... and the formula is the length of a proof built from it
        for log_n, log_b, q, g in ((2, 1, 1, 0), (5, 2, 7, 12), (7, 1, 1, 12), (8, 3, 7, 0)):
            ref = fold_ref.fold_proof(orc, log_n, log_b, q, 0, K, g)
            assert len(ref.data) == lib.zk_proof_data_len_fold(log_n, log_b, q, g, K), (K, log_n, log_b, q, g)
    assert lib.zk_proof_data_len_fold(10, 3, 1, 0, 0) == 0 and lib.zk_proof_data_len_fold(10, 3, 1, 0, 4) == 0
    # the sizes DESIGN.md quotes: domain 2^24 with 1 and 32 queries, the reference's size
    assert [lib.zk_proof_data_len_fold(21, 3, 1, 0, K) for K in (1, 2, 3)] == [23280, 23560, 31008]
    assert [lib.zk_proof_data_len_fold(21, 3, 32, 0, K) for K in (1, 2, 3)] == [719044, 739164, 981964]
    assert [lib.zk_proof_data_len_fold(10, 3, 1, 0, K) for K in (1, 2, 3)] == [7836, 7976, 10188]


SIZES = [(2, 1), (4, 2), (5, 2), (7, 3), (10, 3)]           # log_n % K != 0 for K = 2 (5, 7) and K = 3 (2, 4, 5, 7, 10)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_cpu_verifier_accepts_reference_proofs(zk, orc, K, hash_kind):
    lib = zk.load()
    for log_n, log_b in SIZES:
        for q, g in ((1, 0), (3, 8)):
            ref = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, g)
            args = (log_n, log_b, ref.public_last, hash_kind, q, g, K)
            assert fold_ref.verify(orc, ref.data, ref.state, *args) == 0          # checked by something that is not the library
            assert fold_ref.verify(orc, ref.data, None, *args) == 0
            assert _check(lib, ref.data, ref.state, *args) == 0
            assert _check(lib, ref.data, None, *args) == 0
            p = zk.Proof(ref.state, ref.data, log_n, log_b, ref.public_last, ("sha256", "field")[hash_kind], q, g, K)
            p.verify()
            p.verify(strict=True)
            assert p.check() == 0 and p.check(strict=True) == 0
            for wrong in {1, 2, 3} - {K}:
                if fold_ref.groups(log_n, wrong) == fold_ref.groups(log_n, K):
                    continue                                # log_n = 2: K = 2 and K = 3 are the same format
                args_w = args[:-1] + (wrong,)
                for st in (ref.state, None):
                    got = _check(lib, ref.data, st, *args_w)
                    assert got != 0 and got == fold_ref.verify(orc, ref.data, st, *args_w), (log_n, log_b, q, g, wrong)


def _tamper_offsets(log_n, log_b, q, g, K):
    """(label, byte offset) of one byte of each kind of field: a beta, a group root, the free term, and in the first query each of
    the s values and one node and the count of each of the s paths of the first, a middle and the last group."""
    L = log_n + log_b
    grp = fold_ref.groups(log_n, K)
    G = len(grp)
    out = [("f_root", 3), ("alpha1", 37), ("cp_root", 50), ("beta0", 76), (f"beta{G - 1}", 76 + 36 * (G - 1) + 1),
           ("root0", 80 + 5), (f"root{G - 1}", 80 + 36 * (G - 1) + 31), ("free_term", 76 + 36 * G)]
    pos = 76 + 36 * G + 4
    if g:
        out.append(("nonce", pos + 2))
        pos += 8
    out.append(("query_raw0", pos))
    pos += 4 * q
    for i in range(4):
        out += [(f"f{i}.value", pos), (f"f{i}.count", pos + 4), (f"f{i}.node", pos + 12 + 32 * (i % L) + 7)]
        pos += 12 + 32 * L
    for j, (r0, steps) in enumerate(grp):
        s, pl = 1 << steps, L - r0
        if j in (0, G // 2, G - 1):
            for t in range(s):
                out.append((f"g{j}.v{t}", pos + 4 * t + (t % 4)))
                base = pos + 4 * s + t * (8 + 32 * pl)
                out += [(f"g{j}.count{t}", base), (f"g{j}.path{t}", base + 8 + 32 * ((t + j) % pl) + 9)]
        pos += s * (12 + 32 * pl)
    return out


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_tampered_proofs_get_the_python_verifiers_number(zk, orc, K, hash_kind):
    lib = zk.load()
    seen = set()
    for log_n, log_b, q, g in ((7, 2, 2, 0), (5, 1, 1, 8), (10, 3, 1, 0)):
        ref = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, g)
        args = (log_n, log_b, ref.public_last, hash_kind, q, g, K)
        variants = [(label, ref.data[:off] + bytes([ref.data[off] ^ 0x04]) + ref.data[off + 1:]) for label, off in _tamper_offsets(log_n, log_b, q, g, K)]
        variants += [("trailing", ref.data + b"\0"), ("truncated", ref.data[:-1]), ("truncated_header", ref.data[:60])]
        for label, data in variants:
            for st in (ref.state, None):
                want = fold_ref.verify(orc, data, st, *args)
                got = _check(lib, data, st, *args)
                assert got == want, (label, st is not None, got, want)
                # not strict: the nonce is skipped unchecked, and (as in proof.rs) nothing is opened under the last layer's root
                assert want != 0 or (st is None and label in ("nonce", f"root{len(fold_ref.groups(log_n, K)) - 1}")), label
                seen.add(want)
        for last in (ref.public_last + 1, ref.public_last ^ 0x80000000):
            assert _check(lib, ref.data, None, log_n, log_b, last, *args[3:]) == fold_ref.verify(orc, ref.data, None, log_n, log_b, last, *args[3:]) != 0
    # every family of check numbers was reached
    assert {-1, -2, -4, -7, -8, -100, -300, -400, -1999}.issubset(seen) and any(c <= -1001 for c in seen), sorted(seen)
    assert any(-300 < c <= -200 for c in seen)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q", [(4, 1, 1), (5, 2, 2)])
def test_k1_gives_every_input_the_number_of_zk_verify_grind(zk, orc, log_n, log_b, q, hash_kind):
    lib = zk.load()
    for it in verify_corpus.corpus(orc, log_n, log_b, q, hash_kind):
        for st in (it.state, None):
            want = C.c_int32(777)
            lib.zk_verify_grind(it.data, len(it.data), st, log_n, log_b, it.public_last, hash_kind, q, 0, C.byref(want))
            assert _check(lib, it.data, st, log_n, log_b, it.public_last, hash_kind, q, 0, 1) == want.value, it.label
    # ... and with a nonce: the grinding proofs of grind_ref, valid and with a nonce that misses the bits
    import grind_ref
    data, state, last, w = grind_ref.grind_proof(orc, log_n, log_b, q, hash_kind, 8)
    bad = grind_ref.grind_proof(orc, log_n, log_b, q, hash_kind, 8, nonce=next(x for x in range(w + 1, w + 99) if not grind_ref.meets(
        grind_ref.replay_prefix(data, log_n), 8, x)))
    for d, s in ((data, state), (bad[0], bad[1])):
        for st in (s, None):
            want = C.c_int32(777)
            lib.zk_verify_grind(d, len(d), st, log_n, log_b, last, hash_kind, q, 8, C.byref(want))
            assert _check(lib, d, st, log_n, log_b, last, hash_kind, q, 8, 1) == want.value


def test_argument_errors(zk):
    lib = zk.load()
    out = C.c_int32(777)
    data = bytes(100)
    for K in (0, 4):
        assert lib.zk_verify_fold(data, len(data), None, 5, 2, 0, 0, 1, 0, K, C.byref(out)) == -1 and out.value == 777
    assert lib.zk_verify_fold(None, 100, None, 5, 2, 0, 0, 1, 0, 2, C.byref(out)) == -1
    assert lib.zk_verify_fold(data, len(data), None, 5, 2, 0, 2, 1, 0, 2, C.byref(out)) == -1 and out.value == 777
    assert lib.zk_verify_fold(data, len(data), None, 5, 2, 0, 0, 1, 0, 2, None) == -1
    # the setters take no handle on a machine without a GPU: a null one is refused
    assert lib.zk_ctx_set_fold(None, 2) == -1 and lib.zk_ctx_get_fold(None) == 0
    assert lib.zk_fri_fold_multi(None, 0, 2, 1) == -1 and lib.zk_dev_fri_fold_multi(None, None, None, 4, 0, 2, 1, None) == -1
