"""Early stop of FRI in the batched prover (zk_batch_set_fri_stop): zk_batch_prove against the proofs tests/stop_ref.py
builds without the library -- bytes, state, public input -- against the one-call prover with the same stop, and through the batched
GPU verifier.  The final polynomials of a batch come from fri_final_poly_batch_kernel (4096 / M layers of M values per workgroup)."""
import ctypes as C
import threading

import numpy as np
import pytest

import stop_ref
from transforms_ref import P

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER, ERR_CHECK = -1, -4, -5, -7
SEED = 3141592


def _same(p, ref):
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _seeds(batch, first=SEED):
    return [1] * batch, [first + p for p in range(batch)]


def _trace(zk, log_n, a1):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


# ---- 1. proofs are the reference's ------------------------------------------------------------------------------------------------
# (log_n, log_b, D, log_batch, ((q, grind_bits), ...)):
#   (4, 1, 1, 1)   M = 4: two proofs in a workgroup that is nearly empty
#   (4, 1, 3, 1)   R' = 1: a single group of one round at every K, and no FRI tree at all after cp's
#   (5, 2, 2, 5)   q = 1, 7; with K = 3 and coset leaves the 3 rounds make exactly one group
#   (7, 2, 4, 3)   grinding of 12 bits on q = 7
#   (10, 3, 8, 2)  M = 2048: two proofs per workgroup
SHAPES = [(4, 1, 1, 1, ((1, 0),)), (4, 1, 3, 1, ((1, 0),)), (5, 2, 2, 5, ((1, 0), (7, 0))), (7, 2, 4, 3, ((7, 12),)), (10, 3, 8, 2, ((1, 0),))]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("log_n,log_b,D,log_batch,qgs", SHAPES, ids=["M4", "one-round", "q1-q7", "grind", "M2048"])
def test_batch_stop_proofs_are_the_reference(zk, orc, log_n, log_b, D, log_batch, qgs, K, coset, hash_kind):
    """Proof p of the batch is stop_ref's proof of fibsq(1, 3141592 + p): bytes, state, public input; it passes the strict CPU
    verifier and has the length zk_proof_data_len_stop gives; host tree levels on and off give the same bytes.  At log_n 10 the
    Python reference is taken for proofs 0 and batch - 1, and every proof is compared with the one-call prover."""
    lib, nb = zk.load(), 1 << log_batch
    made = {}
    for q, g in qgs:
        with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset,
                             stop_log=D) as bc:
            assert bc.stop_log == D and lib.zk_batch_get_fri_stop(bc._h) == D
            bc.gen_fibsq(*_seeds(nb))
            per_levels = []
            for on in (1, 0):
                assert lib.zk_batch_set_host_levels(bc._h, on) == 0
                per_levels.append(bc.prove())
            for a, b in zip(*per_levels):
                assert a.data == b.data and a.state == b.state
            made[q, g] = per_levels[0]
            plen = lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, int(coset), D)
            assert plen == bc.proof_len == stop_ref.proof_len(log_n, log_b, q, g, K, coset, D)
            assert all(len(p.data) == plen and p.stop_log == D for p in per_levels[0])
    for p in (range(nb) if log_n <= 7 else (0, nb - 1)):     # one committed() per p, shared by its (q, g)
        for q, g in qgs:
            ref = stop_ref.stop_proof(orc, log_n, log_b, q, hash_kind, K, coset, D, g, a1=SEED + p)
            got = made[q, g][p]
            _same(got, ref)
            assert (got.fold_log, got.queries, got.grind_bits, got.coset_leaves, got.stop_log) == (K, q, g, coset, D)
    if log_n > 7:
        for q, g in qgs:
            with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D) as ctx:
                for p in range(nb):
                    _same(made[q, g][p], ctx.prove(_trace(zk, log_n, SEED + p)))
    for proofs in made.values():
        for got in proofs:
            assert got.check(strict=True) == 0


# ---- 2. workgroup boundaries --------------------------------------------------------------------------------------------------------
def test_batch_stop_four_full_workgroups(zk, orc):
    """1024 proofs of M = 16: 256 per workgroup, four full workgroups.  Every proof is the one-call prover's; proofs 0, 255, 256 and
    1023 (the first and last of workgroups 0 and 1, and the last of all) are stop_ref's as well."""
    log_n, log_b, D, log_batch = 5, 2, 2, 10
    nb = 1 << log_batch
    with zk.BatchContext(log_n, log_b, log_batch, stop_log=D) as bc:
        bc.gen_fibsq(*_seeds(nb))
        proofs = bc.prove()
    assert len(proofs) == nb
    with zk.Context(log_n, log_b, stop_log=D) as ctx:
        for p, got in enumerate(proofs):
            _same(got, ctx.prove(_trace(zk, log_n, SEED + p)))
    for p in (0, 255, 256, 1023):
        _same(proofs[p], stop_ref.stop_proof(orc, log_n, log_b, 1, 0, 1, False, D, a1=SEED + p))
        assert proofs[p].check(strict=True) == 0


@pytest.mark.parametrize("K,coset", [(1, False), (3, True)])
def test_batch_stop_largest_layer(zk, K, coset):
    """M = 4096, one proof per workgroup: the largest layer the limits admit, and R' = 1."""
    log_n, log_b, D, log_batch = 9, 4, 8, 1
    with zk.BatchContext(log_n, log_b, log_batch, fold_log=K, coset_leaves=coset, stop_log=D) as bc:
        bc.gen_fibsq(*_seeds(2))
        proofs = bc.prove()
    with zk.Context(log_n, log_b, fold_log=K, coset_leaves=coset, stop_log=D) as ctx:
        for p, got in enumerate(proofs):
            _same(got, ctx.prove(_trace(zk, log_n, SEED + p)))
            assert got.check(strict=True) == 0


# ---- 3. ... and the one-call prover's, on handed-over traces ------------------------------------------------------------------------
@pytest.mark.parametrize("K,log_n,log_b,D", [(1, 8, 2, 3), (2, 10, 3, 5), (3, 7, 2, 1)])
def test_batch_stop_equals_the_single_prover(zk, K, log_n, log_b, D):
    """Traces handed over from the host; every proof equals Context(fold_log=K, stop_log=D).prove of its trace.  log_batch 0 runs on
    the one-call prover itself (a batch of one forwards the option to its context)."""
    q = 3
    with zk.Context(log_n, log_b, queries=q, fold_log=K, stop_log=D) as ctx:
        for log_batch in (0, 3, 4):
            traces = np.stack([_trace(zk, log_n, 5 + 31 * log_batch + p) for p in range(1 << log_batch)])
            with zk.BatchContext(log_n, log_b, log_batch, queries=q, fold_log=K, stop_log=D) as bc:
                assert zk.load().zk_batch_get_fri_stop(bc._h) == D
                bc.set_traces(traces)
                proofs = bc.prove()
            assert len(proofs) == 1 << log_batch
            for p, got in enumerate(proofs):
                _same(got, ctx.prove(traces[p]))
                assert got.fold_log == K and got.stop_log == D and got.check(strict=True) == 0


# ---- 4. the per-proof degree check ---------------------------------------------------------------------------------------------------
def test_batch_stop_degree_check_names_the_proof(zk):
    """All four proofs share one workgroup of the final-polynomial kernel (M = 32); the counts stay per proof, and the lowest broken
    proof is the one reported."""
    log_n, log_b, D, log_batch, q = 8, 2, 3, 2, 2
    lib = zk.load()
    good = np.stack([_trace(zk, log_n, 9 + p) for p in range(1 << log_batch)])
    with zk.BatchContext(log_n, log_b, log_batch, queries=q, stop_log=D) as bc, zk.Context(log_n, log_b, queries=q, stop_log=D) as ctx:
        for broken, who in (((2,), "proof 2"), ((1, 3), "proof 1")):
            traces = good.copy()
            for p in broken:
                traces[p, 100] = (int(traces[p, 100]) + 1) % P
            bc.set_traces(traces)
            with pytest.raises(zk.ZkError, match=who + r" of the batch: final FRI layer has degree >= 2\^3") as e:
                bc.prove()
            assert e.value.code == ERR_CHECK
        bc.set_traces(good)
        for p, got in enumerate(bc.prove()):
            _same(got, ctx.prove(good[p]))
        plen = lib.zk_proof_data_len_stop(log_n, log_b, q, 0, 1, 0, D)
        assert plen == bc.proof_len and plen != lib.zk_proof_data_len_fold(log_n, log_b, q, 0, 1)
        data = np.zeros((bc.batch, plen), dtype=np.uint8)
        states = np.zeros((bc.batch, 32), dtype=np.uint8)
        rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen - 1, states.ctypes.data_as(C.c_void_p))
        assert rc == ERR_BUFFER and str(plen).encode() in lib.zk_last_error()
        assert lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p)) == 0
        assert (data == bc.prove_raw()[0]).all()


# ---- 5. made by the batch, checked by the GPU verifier -------------------------------------------------------------------------------
def test_batch_stop_proofs_pass_the_gpu_verifier(zk):
    log_n, log_b, K, D, q = 10, 3, 3, 6, 3
    with zk.BatchContext(log_n, log_b, 5, queries=q, fold_log=K, coset_leaves=True, stop_log=D) as bc:
        bc.gen_fibsq(*_seeds(32))
        proofs = bc.prove()
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, coset_leaves=True, stop_log=D) as v:
        for strict in (True, False):
            got = v.verify(proofs, strict=strict)
            assert len(got) == 32 and not got.any(), got
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as full:
        with pytest.raises(zk.ZkError, match="proof 0 was made with stop_log 6, this verifier is set to stop_log 0"):
            full.verify(proofs)


# ---- 6. one live batch across settings -------------------------------------------------------------------------------------------------
def test_one_batch_goes_through_stops_factors_and_leaf_formats(zk, orc):
    """Stale gather buffer sizes and stale skipped-tree bits would show in the walk.  Its first step allocates the multi-fold work
    buffer, which is never given back, so a second, fresh batch goes (0, 1, off) -> (2, 1, off): D > 0 at K = 1 without coset leaves on
    a batch that has only made plain K = 1 proofs is where a missing work buffer would show."""
    log_n, log_b, log_batch, q = 7, 2, 2, 2
    L, nb, lib = log_n + log_b, 1 << log_batch, zk.load()
    A, B = _seeds(nb), _seeds(nb, 271828)
    walk = ((4, 3, True), (0, 1, False), (2, 1, False), (0, 2, True), (5, 2, False), (1, 1, True))
    with zk.BatchContext(log_n, log_b, log_batch, queries=q) as bc:
        assert bc.stop_log == 0 and lib.zk_batch_get_fri_stop(bc._h) == 0
        for i, (D, K, coset) in enumerate(walk):
            a0s, a1s = (A, B)[i % 2]
            bc.set_fri_stop(D)
            bc.set_fold(K)
            bc.set_coset_leaves(coset)
            assert lib.zk_batch_get_fri_stop(bc._h) == D == bc.stop_log
            assert lib.zk_batch_get_fold(bc._h) == K and lib.zk_batch_get_coset_leaves(bc._h) == int(coset)
            bc.gen_fibsq(a0s, a1s)
            proofs = bc.prove()
            for p, got in enumerate(proofs):
                ref = stop_ref.stop_proof(orc, log_n, log_b, q, 0, K, coset, D, a1=a1s[p])
                _same(got, ref)
                assert (got.fold_log, got.coset_leaves, got.stop_log) == (K, coset, D) and got.check(strict=True) == 0
                if (D, K, coset) == (0, 1, False):           # every id is materialised again, with full-size heaps
                    for t in range(log_n + 2):
                        m = (1 << L) >> max(t - 1, 0)
                        heap = bc.merkle_nodes(t)
                        assert len(heap) == 2 * nb * m - 1 and bytes(heap[nb - 1 + p]) == ref.c.roots[t], (p, t)
            if D:
                Rp = log_n - D
                for t in (1 + Rp, log_n + 1):
                    with pytest.raises(zk.ZkError, match=f"tree {t} .*fold_log {K}, fri_stop {D}") as e:
                        bc.merkle_nodes(t)
                    assert e.value.code == ERR_STATE
                assert len(bc.merkle_nodes(0, 0, 1)) == 1
    with zk.BatchContext(log_n, log_b, log_batch, queries=q) as fresh:
        for D in (0, 2):
            fresh.set_fri_stop(D)
            fresh.gen_fibsq(*A)
            for p, got in enumerate(fresh.prove()):
                _same(got, stop_ref.stop_proof(orc, log_n, log_b, q, 0, 1, False, D, a1=A[1][p]))


# ---- 7. limits and state ---------------------------------------------------------------------------------------------------------------
def test_batch_stop_limits(zk):
    lib = zk.load()
    with zk.BatchContext(5, 2, 1) as bc:
        bc.set_fri_stop(2)
        for D in (5, 9):                                     # D > log_n - 1; D > 8
            assert lib.zk_batch_set_fri_stop(bc._h, D) == ERR_INVALID
            assert b"zk_batch_set_fri_stop: need stop_log <= 8" in lib.zk_last_error()
            assert lib.zk_batch_get_fri_stop(bc._h) == 2
        assert lib.zk_batch_set_fri_stop(bc._h, 2) == 0 and lib.zk_batch_set_fri_stop(bc._h, 4) == 0
        assert lib.zk_batch_get_fri_stop(bc._h) == 4
    with zk.BatchContext(12, 5, 1) as bc:
        assert lib.zk_batch_set_fri_stop(bc._h, 8) == ERR_INVALID    # D + log_blowup > 12
        assert lib.zk_batch_get_fri_stop(bc._h) == 0
        assert lib.zk_batch_set_fri_stop(bc._h, 7) == 0 and lib.zk_batch_get_fri_stop(bc._h) == 7
    with zk.BatchContext(5, 2, 0) as one:                    # a batch of one: the context's limits, through the forward
        assert lib.zk_batch_set_fri_stop(one._h, 5) == ERR_INVALID and lib.zk_batch_get_fri_stop(one._h) == 0
        assert lib.zk_batch_set_fri_stop(one._h, 3) == 0 and lib.zk_batch_get_fri_stop(one._h) == 3


def test_set_fri_stop_is_refused_while_a_prove_runs(zk):
    """The shape of test_set_coset_leaves_is_refused_while_a_prove_runs: zk_batch_set_fri_stop from a second thread answers
    ZK_ERR_STATE while a zk_batch_prove holds the batch, and the proofs of that run are unharmed."""
    lib = zk.load()
    log_n, log_b, log_batch, D = 16, 3, 4, 4
    with zk.BatchContext(log_n, log_b, log_batch, stop_log=D) as bc:
        bc.gen_fibsq(*_seeds(1 << log_batch))
        first, _ = bc.prove_raw()
        seen, out, stop = [], {}, threading.Event()

        def prover():
            done = 0
            try:
                while done < 6:
                    try:
                        out["last"] = bc.prove_raw()[0]
                        done += 1
                    except zk.ZkError as e:                 # the setter of the other thread held the batch at that instant
                        assert e.code == ERR_STATE
                        seen.append(ERR_STATE)
            finally:
                stop.set()                                  # whatever happened here, the other thread stops calling

        t = threading.Thread(target=prover)
        t.start()
        while not stop.is_set():
            seen.append(lib.zk_batch_set_fri_stop(bc._h, D))   # the stop it already has: accepted when idle, and changes nothing
        t.join()
        assert ERR_STATE in seen
        assert set(seen) <= {0, ERR_STATE}
        assert (out["last"] == first).all()
        assert lib.zk_batch_set_fri_stop(bc._h, D) == 0 and lib.zk_batch_get_fri_stop(bc._h) == D
        again, _ = bc.prove_raw()
        assert (again == first).all()
