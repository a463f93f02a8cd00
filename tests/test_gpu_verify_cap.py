"""Batched verification of proofs with Merkle caps on the GPU (zk_verifier_set_merkle_cap, Verifier(cap_log=c)): every element of
checks_out is the number the CPU verifier zk_verify_cap gives for that proof -- for batches of 64 valid proofs built without the library
(tests/cap_ref.py) at every setting the cap combines with, for the tamper corpus (tests/verify_cap_corpus.py), for proofs of another
cap, and for one handle whose cap changes between runs; then one round trip from the library's prover."""
import numpy as np
import pytest

import cap_ref
import verify_cap_corpus
import verify_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}


def _gpu(v, items, strict, stride=None):
    plen = len(items[0].data)
    data = np.zeros((len(items), stride or plen), dtype=np.uint8)
    for r, it in enumerate(items):
        data[r, :plen] = np.frombuffer(it.data, dtype=np.uint8)
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
    return v.verify_raw(data, [it.public_last for it in items], states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("c", [1, 4, 8])
@pytest.mark.parametrize("log_n,log_b", [(6, 3), (10, 3)])
def test_valid_proofs_are_accepted(zk, orc, log_n, log_b, c, hash_kind):
    """K in {1, 3}, one-value and coset leaves, D in {0, 2}: a batch of 64 (one full wave) of the two reference proofs in turn, the
    last one with a byte of its last path flipped so that an accepted batch is not a verifier that accepts everything."""
    lib = zk.load()
    n = 0
    for K in (1, 3):
        for coset in (False, True):
            for D in (0, 2):
                q, g = ((2, 0), (3, 4))[n & 1]
                n += 1
                proofs = verify_cap_corpus.ref_proofs(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)
                items = [verify_corpus.Item(f"p{i}", *proofs[i & 1]) for i in range(64)]
                d = bytearray(items[63].data)
                d[-5] ^= 4
                items[63] = verify_corpus.Item("p63.bad", bytes(d), items[63].state, items[63].public_last)
                with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D,
                                 cap_log=c) as v:
                    assert v.proof_len == len(items[0].data) == cap_ref.proof_len(log_n, log_b, q, g, K, coset, D, c)
                    assert lib.zk_verifier_get_merkle_cap(v._h) == c and v.cap_log == c
                    for strict in (True, False):
                        cpu = verify_cap_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, c, hash_kind, strict)
                        got = _gpu(v, items, strict)
                        what = (K, coset, D, q, g, strict)
                        assert (cpu[:63] == 0).all() and cpu[63] != 0, (what, cpu)
                        assert np.array_equal(got, cpu), (what, _mismatches(items, got, cpu))


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K,coset,D,c", verify_cap_corpus.SHAPES)
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_cap's number.  A cap entry
    no path lands in passes the plain run and fails the strict one."""
    items = verify_cap_corpus.corpus(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c) as v:
        res = {}
        for strict in (True, False):
            want = verify_cap_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, g, K, coset, D, c, hash_kind, strict)
            got = res[strict] = _gpu(v, items, strict, stride=len(items[0].data) + (0 if strict else 5))
            print(f"shape {(log_n, log_b, q, g, K, coset, D, c)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{len(set(want.tolist()))} distinct check numbers, {(got != want).sum()} mismatches")
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
        assert (res[True] != 0).sum() > len(items) // 2
        for i, it in enumerate(items):
            if it.label.startswith("p0.") and ".landed." in it.label and not it.label.endswith("swap"):
                assert res[False][i] != 0, it.label
            if it.label.startswith("p0.") and ".free." in it.label:
                assert res[False][i] == 0 and res[True][i] <= -1000, (it.label, res[False][i], res[True][i])


def test_a_proof_of_another_cap(zk, orc):
    """(6, 3, q = 2): c = 2 proofs read by a c = 4 verifier and by a c = 0 one, cut or zero-padded to the verifier's length: the number
    zk_verify_cap of the verifier's settings gives those bytes (-1 by length on the CPU), and Verifier.verify names the difference."""
    log_n, log_b, q = 6, 3, 2
    proofs = verify_cap_corpus.ref_proofs(orc, log_n, log_b, q, 0, 1, False, 0, 2, 0)
    for v_c in (4, 0):
        with zk.Verifier(log_n, log_b, queries=q, cap_log=v_c) as v:
            plen = v.proof_len
            assert plen != len(proofs[0][0])
            items = [verify_corpus.Item(f"p{i}", (d + bytes(plen))[:plen], s, last) for i, (d, s, last) in enumerate(proofs)]
            for strict in (True, False):
                want = verify_cap_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, 0, 1, False, 0, v_c, 0, strict)
                got = _gpu(v, items, strict)
                assert (want != 0).all() and np.array_equal(got, want), (v_c, strict, got, want)
            with pytest.raises(zk.ZkError) as err:
                v.verify([zk.Proof(s, d, log_n, log_b, last, queries=q, cap_log=2) for d, s, last in proofs])
            assert "cap_log" in str(err.value)


def test_one_handle_changes_cap(zk, orc):
    """c = 0 -> 4 -> 0 -> 1 on one handle with (K 3, coset, D 2): each run reads the format of the current setting; c = 9 is refused and
    leaves the setting as it was; a null handle is refused."""
    lib = zk.load()
    log_n, log_b, q, K, coset, D = 6, 3, 2, 3, True, 2
    assert lib.zk_verifier_set_merkle_cap(None, 1) == -1 and lib.zk_verifier_get_merkle_cap(None) == 0
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, coset_leaves=coset, stop_log=D) as v:
        for c in (0, 4, 0, 1):
            v.set_merkle_cap(c)
            assert lib.zk_verifier_set_merkle_cap(v._h, 9) == -1 and lib.zk_verifier_get_merkle_cap(v._h) == c
            items = verify_cap_corpus.corpus(orc, log_n, log_b, q, 0, K, coset, D, c, 0)
            assert v.proof_len == len(items[0].data)
            for strict in (True, False):
                want = verify_cap_corpus.cpu_checks(lib, items, log_n, log_b, q, 0, K, coset, D, c, 0, strict)
                got = _gpu(v, items, strict)
                assert np.array_equal(got, want), (c, strict, _mismatches(items, got, want))


def test_prover_to_verifier_round_trip(zk):
    """(10, 3), c = 5, K = 2, coset leaves, three queries: what Context.prove makes, Verifier.verify accepts, strict and not, and a
    flipped byte in one proof is that proof's rejection alone."""
    log_n, log_b, c = 10, 3, 5
    kw = dict(queries=3, fold_log=2, coset_leaves=True, cap_log=c)
    with zk.Context(log_n, log_b, **kw) as ctx, zk.Verifier(log_n, log_b, **kw) as v:
        proofs = [ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, a1)) for a1 in (3141592, 3141593, 3141594)]
        assert all(p.cap_log == c and p.check(strict=True) == 0 for p in proofs)
        for strict in (True, False):
            assert (v.verify(proofs, strict=strict) == 0).all()
        d = bytearray(proofs[1].data)
        d[len(d) // 2] ^= 1
        bad = zk.Proof(proofs[1].state, bytes(d), log_n, log_b, proofs[1].public_last, **kw)
        got = v.verify([proofs[0], bad, proofs[2]])
        assert got[0] == 0 and got[2] == 0 and got[1] == bad.check(strict=True) != 0
