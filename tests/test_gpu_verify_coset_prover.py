"""The batched GPU verifier on the coset-leaf proofs of the library's own prover (Context(coset_leaves=True)): the round trip at
the reference's size for K = 1, 2, 3 with one tampered proof, and two proofs at domain 2^24."""
import numpy as np
import pytest

import verify_coset_corpus

pytestmark = pytest.mark.gpu


def _arrays(proofs):
    data = np.stack([np.frombuffer(p.data, dtype=np.uint8) for p in proofs]).copy()
    states = np.stack([np.frombuffer(p.state, dtype=np.uint8) for p in proofs]).copy()
    return data, states, np.array([p.public_last & 0xFFFFFFFF for p in proofs], dtype=np.uint32)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_round_trip_with_the_prover(zk, K):
    """64 proofs from Context(10, 3, coset_leaves=True, fold_log=K): accepted strict and plain, through verify() and verify_raw();
    then one flipped byte in proof 37 gives Proof.check's number for it and 0 for all the others."""
    with zk.Context(10, 3, fold_log=K, coset_leaves=True) as ctx:
        proofs = [ctx.prove(zk.trace_fibsq(1023, 1, 3141592 + p)) for p in range(64)]
    assert all(p.coset_leaves and p.fold_log == K for p in proofs)
    data, states, last = _arrays(proofs)
    with zk.Verifier(10, 3, fold_log=K, coset_leaves=True) as v:
        assert data.shape[1] == v.proof_len
        for strict in (True, False):
            assert (v.verify(proofs, strict=strict) == 0).all()
        assert (v.verify_raw(data, last, states) == 0).all()
        data[37, data.shape[1] // 2] ^= 0x20
        for strict in (True, False):
            got = v.verify_raw(data, last, states if strict else None)
            want = zk.Proof(states[37].tobytes(), data[37].tobytes(), 10, 3, int(last[37]), fold_log=K, coset_leaves=True).check(strict)
            assert want != 0 and got[37] == want, (strict, got[37], want)
            assert (np.delete(got, 37) == 0).all()


@pytest.mark.parametrize("q", [1, 16])
def test_benchmark_domain_2e24(zk, q):
    """Two 2^24 proofs (log_n 21) with coset leaves folded by 8: accepted; a tampered node of the path of the last group (G = 7:
    j = 6) gives the CPU's -1999 strict and -306 plain."""
    log_n, log_b, K = 21, 3, 3
    with zk.Context(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as ctx:
        proofs = [ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, a1)) for a1 in (3141592, 3141593)]
    data, states, last = _arrays(proofs)
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as v:
        assert data.shape[1] == v.proof_len
        assert (v.verify_raw(data, last, states) == 0).all()
        assert (v.verify_raw(data, last) == 0).all()
        off = [o for n, o, _, _ in verify_coset_corpus.fields(log_n, log_b, q, 0, K) if n.startswith("q0.group6.node")][0]
        bad = data.copy()
        bad[1, off + 7] ^= 0x04
        for strict in (True, False):
            got = v.verify_raw(bad, last, states if strict else None)
            cpu = zk.Proof(states[1].tobytes(), bad[1].tobytes(), log_n, log_b, int(last[1]), queries=q, fold_log=K, coset_leaves=True).check(strict)
            assert got[0] == 0 and got[1] == cpu
            assert cpu == (-1999 if strict else -306)
