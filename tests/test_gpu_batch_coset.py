"""Coset leaves in the batched prover (zk_batch_set_coset_leaves): zk_batch_prove against the proofs
tests/coset_ref.py builds without the library -- bytes, state, public input, every node of every committed tree -- against the
one-call prover with coset leaves, and through the batched GPU verifier."""
import ctypes as C

import numpy as np
import pytest

import coset_ref
import fold_ref
from transforms_ref import P, require_memory

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER, ERR_CHECK = -1, -4, -5, -7
SEED = 3141592


def _same(p, ref):
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _seeds(batch, first=SEED):
    return [1] * batch, [first + p for p in range(batch)]


def _subtree(heap, log_batch, p, log_m):
    """Proof p's tree (2 * 2^log_m - 1 nodes, heap order) out of the batch heap."""
    rows = [heap[(1 << (log_batch + d)) - 1 + (p << d):(1 << (log_batch + d)) - 1 + ((p + 1) << d)] for d in range(log_m + 1)]
    return np.concatenate(rows)


# ---- 1. trees, node for node ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_kind,log_n,log_b,log_batch", [(0, 4, 1, 1), (0, 5, 2, 3), (1, 7, 1, 2), (0, 10, 3, 2)])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_batch_coset_trees_node_for_node(zk, orc, K, hash_kind, log_n, log_b, log_batch):
    """Every node of every committed tree of every proof, host-built levels included, by the tree's own heap.  (4, 1) with K = 3
    has per-proof trees of 4 and 2 leaves (a wave of the leaf kernel spans proofs) and a last group of one round; (10, 3, 2) has
    4 096 .. 16 384 leaves in tree 1 of the batch, so a lane of the leaf kernel makes four trips; (1, 7, 1, 2) is the field hash."""
    L, nb = log_n + log_b, 1 << log_batch
    refs = [coset_ref.committed(orc, log_n, log_b, hash_kind, K, SEED + p) for p in range(nb)]
    steps = refs[0].steps
    committed = sorted(steps)
    assert committed == sorted({0, 1} | {1 + r0 + s for r0, s in fold_ref.groups(log_n, K)})
    assert steps[0] == 0 and steps[1 + log_n] == 0 and steps[1] == min(K, log_n)
    with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[hash_kind], fold_log=K, coset_leaves=True) as bc:
        assert bc.coset_leaves and zk.load().zk_batch_get_coset_leaves(bc._h) == 1
        bc.gen_fibsq(*_seeds(nb))
        proofs = bc.prove()
        heaps = {}
        for i in committed:
            m = ((1 << L) >> max(i - 1, 0)) >> steps[i]      # leaves of one proof's tree
            heaps[i] = bc.merkle_nodes(i, coset_steps=steps[i])
            assert len(heaps[i]) == 2 * nb * m - 1, i
            if steps[i]:                                     # one past the coset heap
                for first, count in ((2 * nb * m - 1, 1), (0, 2 * nb * m), (2 * nb * m - 2, 2)):
                    with pytest.raises(zk.ZkError) as e:
                        bc.merkle_nodes(i, first, count)
                    assert e.value.code == ERR_INVALID, (i, first, count)
                assert len(bc.merkle_nodes(i, 2 * nb * m - 2, 1)) == 1
        for i in range(log_n + 2):
            if i not in steps:
                for call in (lambda: bc.merkle_nodes(i), lambda: bc.merkle_nodes(i, 0, 1)):
                    with pytest.raises(zk.ZkError, match=f"tree {i} .*fold_log {K}") as e:
                        call()
                    assert e.value.code == ERR_STATE
    assert (len(committed) < log_n + 2) == (K > 1)
    for p in range(nb):
        assert proofs[p].public_last == refs[p].public_last
        for i in committed:
            log_m = (L if i == 0 else L - (i - 1)) - steps[i]
            assert bytes(heaps[i][nb - 1 + p]) == refs[p].roots[i], (p, i)
            assert np.array_equal(_subtree(heaps[i], log_batch, p, log_m), refs[p].trees[i]), (p, i)


# ---- 2. proofs are the reference's ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b", [(4, 1), (5, 2), (7, 2), (10, 3)])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_batch_coset_proofs_are_the_reference(zk, orc, K, log_n, log_b, hash_kind):
    """Proof p of every batch (log_batch 1, 3, 5; q = 1, 7; grinding on (10, 3, q = 7)) is coset_ref's proof of
    fibsq(1, 3141592 + p): bytes, state, public input; host tree tops on and off give the same bytes.  At (10, 3) the Python
    reference is taken for proofs 0 and batch - 1 only, and every proof is compared with the one-call prover as well."""
    lib = zk.load()
    made = {}                                                # (log_batch, q) -> proofs
    for log_batch in (1, 3, 5):
        for q in (1, 7):
            g = 12 if (log_n, log_b, q) == (10, 3, 7) else 0
            with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=True) as bc:
                assert bc.fold_log == K and lib.zk_batch_get_fold(bc._h) == K and lib.zk_batch_get_coset_leaves(bc._h) == 1
                bc.gen_fibsq(*_seeds(1 << log_batch))
                per_levels = []
                for on in (1, 0):
                    assert lib.zk_batch_set_host_levels(bc._h, on) == 0
                    per_levels.append(bc.prove())
                for a, b in zip(*per_levels):
                    assert a.data == b.data and a.state == b.state
                made[log_batch, q] = per_levels[0]
                plen = lib.zk_proof_data_len_coset(log_n, log_b, q, g, K)
                assert all(len(p.data) == plen and p.coset_leaves for p in per_levels[0])
    with_ref = range(1 << 5) if log_n <= 7 else sorted({0} | {(1 << lb) - 1 for lb in (1, 3, 5)})
    for p in with_ref:                                       # one committed() per p; the transcript prefix is shared by q = 1, 7
        for q in (1, 7):
            g = 12 if (log_n, log_b, q) == (10, 3, 7) else 0
            ref = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, g, a1=SEED + p)
            for log_batch in (1, 3, 5):
                if p < (1 << log_batch) and (log_n <= 7 or p in (0, (1 << log_batch) - 1)):
                    got = made[log_batch, q][p]
                    _same(got, ref)
                    assert got.fold_log == K and got.queries == q and got.grind_bits == g and got.coset_leaves
    if log_n > 7:
        for q in (1, 7):
            g = 12 if q == 7 else 0
            with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=True) as ctx:
                for p in range(1 << 5):
                    one = ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, SEED + p))
                    for log_batch in (1, 3, 5):
                        if p < (1 << log_batch):
                            _same(made[log_batch, q][p], one)
    for key, proofs in made.items():
        for got in proofs:
            assert got.check(strict=True) == 0


# ---- 3. ... and the one-call prover's, on handed-over traces ------------------------------------------------------------------------
@pytest.mark.parametrize("K,log_n,log_b", [(1, 8, 2), (2, 10, 3), (3, 7, 2)])
def test_batch_coset_equals_the_single_prover(zk, K, log_n, log_b):
    """Traces handed over from the host; every proof equals Context(fold_log=K, coset_leaves=True).prove of its trace.  log_batch 0
    runs on the one-call prover itself (a batch of one forwards the option to its context)."""
    q = 3
    with zk.Context(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as ctx:
        for log_batch in (0, 3, 4):
            traces = np.stack([zk.trace_fibsq((1 << log_n) - 1, 1, 5 + 31 * log_batch + p) for p in range(1 << log_batch)])
            with zk.BatchContext(log_n, log_b, log_batch, queries=q, fold_log=K, coset_leaves=True) as bc:
                assert zk.load().zk_batch_get_coset_leaves(bc._h) == 1
                bc.set_traces(traces)
                proofs = bc.prove()
            assert len(proofs) == 1 << log_batch
            for p, got in enumerate(proofs):
                one = ctx.prove(traces[p])
                _same(got, one)
                assert got.fold_log == K and got.coset_leaves and got.check(strict=True) == 0


# ---- 4. made by the batch, checked by the GPU verifier -------------------------------------------------------------------------------
def test_batch_coset_proofs_pass_the_gpu_verifier(zk):
    log_n, log_b, K, q = 10, 3, 3, 3
    with zk.BatchContext(log_n, log_b, 5, queries=q, fold_log=K, coset_leaves=True) as bc:
        bc.gen_fibsq(*_seeds(32))
        proofs = bc.prove()
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as v:
        for strict in (True, False):
            got = v.verify(proofs, strict=strict)
            assert len(got) == 32 and not got.any(), got
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K) as plain:
        with pytest.raises(zk.ZkError, match="proof 0 was made with coset leaves, this verifier is set to one-value leaves"):
            plain.verify(proofs)


# ---- 5. one live batch across settings -------------------------------------------------------------------------------------------------
def test_one_batch_goes_through_leaf_formats_and_factors(zk, orc):
    """Stale per-tree steps, stale gather buffer sizes and a missing multi-fold work buffer (coset on at K = 1, after a plain K = 1
    proof) would all show here."""
    log_n, log_b, log_batch, q = 7, 2, 2, 2
    L, nb, lib = log_n + log_b, 1 << log_batch, zk.load()
    A, B = _seeds(nb), _seeds(nb, 271828)
    with zk.BatchContext(log_n, log_b, log_batch, queries=q) as bc:
        assert not bc.coset_leaves and lib.zk_batch_get_coset_leaves(bc._h) == 0
        for (coset, K), (a0s, a1s) in zip(((True, 3), (False, 1), (True, 1), (False, 2), (True, 2)), (A, B, A, B, A)):
            bc.set_coset_leaves(coset)
            bc.set_fold(K)
            assert lib.zk_batch_get_coset_leaves(bc._h) == int(coset) and bc.coset_leaves == coset and lib.zk_batch_get_fold(bc._h) == K
            bc.gen_fibsq(a0s, a1s)
            proofs = bc.prove()
            for p, got in enumerate(proofs):
                ref = (coset_ref.coset_proof(orc, log_n, log_b, q, 0, K, a1=a1s[p]) if coset
                       else fold_ref.fold_proof(orc, log_n, log_b, q, 0, K, a1=a1s[p]))
                _same(got, ref)
                assert got.fold_log == K and got.coset_leaves == coset and got.check(strict=True) == 0
                if (coset, K) == (False, 1):                 # every id is materialised again, with full-size heaps
                    for i in range(log_n + 2):
                        m = (1 << L) >> max(i - 1, 0)
                        heap = bc.merkle_nodes(i)
                        assert len(heap) == 2 * nb * m - 1 and bytes(heap[nb - 1 + p]) == ref.c.roots[i], (p, i)
            if K > 1:
                with pytest.raises(zk.ZkError) as e:
                    bc.merkle_nodes(2, 0, 1)
                assert e.value.code == ERR_STATE


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_batch_coset_buffer_and_trace_errors(zk):
    lib = zk.load()
    log_n, log_b, log_batch, K = 8, 2, 2, 2
    with zk.BatchContext(log_n, log_b, log_batch, queries=2, fold_log=K, coset_leaves=True) as bc:
        traces = np.stack([zk.trace_fibsq((1 << log_n) - 1, 1, 9 + p) for p in range(1 << log_batch)])
        bc.set_traces(traces)
        plen = lib.zk_proof_data_len_coset(log_n, log_b, 2, 0, K)
        assert plen != lib.zk_proof_data_len_fold(log_n, log_b, 2, 0, K) and plen == bc.proof_len
        data = np.zeros((bc.batch, plen), dtype=np.uint8)
        states = np.zeros((bc.batch, 32), dtype=np.uint8)
        rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen - 1, states.ctypes.data_as(C.c_void_p))
        assert rc == ERR_BUFFER and str(plen).encode() in lib.zk_last_error()
        assert lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p)) == 0
        assert (data == bc.prove_raw()[0]).all()
        traces[2, 100] = (int(traces[2, 100]) + 1) % P      # a broken trace in one proof of the batch
        bc.set_traces(traces)
        with pytest.raises(zk.ZkError, match="proof 2") as e:
            bc.prove()
        assert e.value.code == ERR_CHECK


def test_set_coset_leaves_is_refused_while_a_prove_runs(zk):
    """The shape of test_set_fold_is_refused_while_a_prove_runs: zk_batch_set_coset_leaves from a second thread answers
    ZK_ERR_STATE while a zk_batch_prove holds the batch, and the proofs of that run are unharmed."""
    import threading
    lib = zk.load()
    log_n, log_b, log_batch, K = 16, 3, 4, 2
    with zk.BatchContext(log_n, log_b, log_batch, fold_log=K, coset_leaves=True) as bc:
        bc.gen_fibsq(*_seeds(1 << log_batch))
        first, _ = bc.prove_raw()
        seen, out, stop = [], {}, threading.Event()

        def prover():
            done = 0
            while done < 6:
                try:
                    out["last"] = bc.prove_raw()[0]
                    done += 1
                except zk.ZkError as e:                     # the setter of the other thread held the batch at that instant
                    assert e.code == ERR_STATE
                    seen.append(ERR_STATE)
            stop.set()

        t = threading.Thread(target=prover)
        t.start()
        while not stop.is_set():
            seen.append(lib.zk_batch_set_coset_leaves(bc._h, 1))   # the format it already has: accepted when idle, and changes nothing
        t.join()
        assert ERR_STATE in seen
        assert set(seen) <= {0, ERR_STATE}
        assert (out["last"] == first).all()
        assert lib.zk_batch_set_coset_leaves(bc._h, 1) == 0 and lib.zk_batch_get_coset_leaves(bc._h) == 1
        again, _ = bc.prove_raw()
        assert (again == first).all()


# ---- 7. domain 2^24 ------------------------------------------------------------------------------------------------------------------------
def test_batch_coset_domain_2e24(zk):
    """Two 2^24 proofs in lockstep, K = 3, SHA-256: each is the one-call prover's of the same trace, and the strict verifier accepts
    both.  (No Python reference at this size.)"""
    log_n, log_b, K = 21, 3, 3
    require_memory(10 << 30, 6 << 30)
    seeds = [SEED, SEED + 1]
    with zk.BatchContext(log_n, log_b, 1, fold_log=K, coset_leaves=True) as bc:
        bc.gen_fibsq([1, 1], seeds)
        proofs = bc.prove()
    with zk.Context(log_n, log_b, fold_log=K, coset_leaves=True) as ctx:
        for p, got in enumerate(proofs):
            _same(got, ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, seeds[p])))
    for p in proofs:
        out = C.c_int32(7)
        assert zk.load().zk_verify_coset(p.data, len(p.data), p.state, log_n, log_b, p.public_last, 0, 1, 0, K, C.byref(out)) == 0 and out.value == 0
