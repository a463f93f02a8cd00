"""Challenges in E = F_P[u] / (u^2 - 5) in the batched prover (zk_batch_set_ext, BatchContext(ext_log=1)): every proof of an
ext batch is the one-call prover's ext proof of the same trace -- bytes, final channel state, public_last -- and the proof tests/ext_ref.py
builds without the library, has the length zk_proof_data_len_ext gives, passes the strict CPU verifier and, a batch at a time, the GPU
verifier with ext_log = 1.  Traces are fibsq(1, SEED + p).  The Python model takes every proof of a batch of <= 32, else the first and
the last."""
import ctypes as C
import threading

import numpy as np
import pytest

import ext_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_CHECK = -1, -4, -7
SEED = 3141592
P = ext_ref.P


def _seeds(batch, first=SEED):
    return [1] * batch, [first + p for p in range(batch)]


def _trace(zk, log_n, a1):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


def _same(p, ref):
    assert len(p.data) == len(ref.data), (len(p.data), len(ref.data))
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _check_batch(zk, orc, proofs, log_n, log_b, K, coset, h, D, c, q, g, first=SEED):
    lib, nb = zk.load(), len(proofs)
    plen = lib.zk_proof_data_len_ext(log_n, log_b, q, g, K, int(coset), D, c, 1)
    assert plen == ext_ref.proof_len(log_n, log_b, q, g, K, coset, D, c)
    with zk.Context(log_n, log_b, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c,
                    ext_log=1) as ctx:
        for p, got in enumerate(proofs):
            _same(got, ctx.prove(_trace(zk, log_n, first + p)))
    for p in (range(nb) if nb <= 32 else (0, nb - 1)):
        _same(proofs[p], ext_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, g, a1=first + p))
    for got in proofs:
        assert len(got.data) == plen and got.ext_log == 1
        assert (got.fold_log, got.queries, got.grind_bits, got.coset_leaves, got.stop_log, got.cap_log) == (K, q, g, coset, D, c)
        assert got.check(strict=True) == 0
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c,
                     ext_log=1) as v:
        res = v.verify(proofs)
        assert len(res) == nb and not np.asarray(res).any(), res


def _check_trees(zk, orc, bc, log_n, log_b, K, coset, h, D, c, proofs_to_check, first=SEED):
    """zk_batch_merkle_nodes of every committed tree from each proof's cap down, and zk_batch_merkle_cap, against the model."""
    lib, lb = zk.load(), bc.log_batch
    for p in proofs_to_check:
        cm = ext_ref.committed(orc, log_n, log_b, h, K, coset, D, c, first + p)
        for tid, heap in cm.trees.items():
            lg, ce = cm.lg[tid], cm.ce[tid]
            steps = cm.lg[0] - max(tid - 1, 0) - lg if tid else 0
            assert lib.zk_batch_merkle_cap_log(bc._h, tid) == ce, tid
            for d in range(ce, lg + 1):
                got = bc.merkle_nodes(tid, (1 << (lb + d)) - 1 + (p << d), 1 << d, coset_steps=steps)
                assert np.array_equal(got, heap[(1 << d) - 1:(2 << d) - 1]), (p, tid, d)
            assert bc.merkle_cap(tid, p).tobytes() == cm.caps[tid], (p, tid)
            if ce:                                           # nothing above the cap was built
                out = np.zeros(32, dtype=np.uint8)
                assert lib.zk_batch_merkle_nodes(bc._h, tid, (1 << (lb + ce)) - 2, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE


def _prove(zk, log_n, log_b, log_batch, K=1, coset=False, h=0, D=0, c=0, q=2, g=0, levels=(None,), after=None):
    lib = zk.load()
    with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D,
                         cap_log=c, ext_log=1) as bc:
        assert bc.ext_log == 1 and lib.zk_batch_get_ext(bc._h) == 1
        assert bc.proof_len == lib.zk_proof_data_len_ext(log_n, log_b, q, g, K, int(coset), D, c, 1)
        bc.gen_fibsq(*_seeds(1 << log_batch))
        runs = []
        for on in levels:
            if on is not None:
                assert lib.zk_batch_set_host_levels(bc._h, on) == 0
            runs.append(bc.prove())
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.data == b.data and a.state == b.state
        if after:
            after(bc)
    return runs[0]


# ---- 1. the shapes ----------------------------------------------------------------------------------------------------------------------
# (2, 1, 1) the smallest, every tree clamped; (5, 2, 5) host levels on, then off; (10, 3, 7) crosses the latency switch of the Merkle
# build with 128 channels on the pool; (6, 2, 0) the batch of one, forwarded to its context
SHAPES = [(2, 1, 1), (4, 2, 3), (5, 2, 5), (10, 3, 7), (6, 2, 0)]


@pytest.mark.parametrize("K,coset", [(1, False), (3, True)], ids=["K1-plain", "K3-coset"])
@pytest.mark.parametrize("log_n,log_b,log_batch", SHAPES, ids=lambda v: str(v))
def test_batch_ext_shapes(zk, orc, log_n, log_b, log_batch, K, coset):
    levels = (1, 0) if (log_n, log_b, log_batch) == (5, 2, 5) else (None,)
    proofs = _prove(zk, log_n, log_b, log_batch, K, coset, levels=levels)
    assert len(proofs) == 1 << log_batch
    _check_batch(zk, orc, proofs, log_n, log_b, K, coset, 0, 0, 0, 2, 0)


# ---- 2. every setting ext combines with ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 3, 8])
@pytest.mark.parametrize("h", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_batch_ext_crossings(zk, orc, K, coset, D, h, c):
    log_n, log_b, log_batch = 5, 2, 3
    proofs = _prove(zk, log_n, log_b, log_batch, K, coset, h, D, c,
                    after=lambda bc: _check_trees(zk, orc, bc, log_n, log_b, K, coset, h, D, c, (0, 7)))
    _check_batch(zk, orc, proofs, log_n, log_b, K, coset, h, D, c, 2, 0)


def test_indices_above_the_cap_are_refused(zk):
    lib = zk.load()
    with zk.BatchContext(5, 2, 3, cap_log=3, ext_log=1) as bc:
        bc.gen_fibsq(*_seeds(8))
        bc.prove()
        out = np.zeros(32 << 3, dtype=np.uint8)
        assert lib.zk_batch_merkle_cap(bc._h, 1, 8, out.ctypes.data_as(C.c_void_p), out.size) == ERR_INVALID     # proof out of range
        assert lib.zk_batch_merkle_nodes(bc._h, 1, 0, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert b"lies above its Merkle cap" in lib.zk_last_error()


@pytest.mark.parametrize("q,g", [(7, 0), (16, 0), (2, 12)], ids=["q7", "q16", "grind12"])
def test_batch_ext_queries_and_grinding(zk, orc, q, g):
    """On the shape whose f cap goes through digest_level_post_kernel: (10, 3, 7) with K = 3, coset leaves and cap 8."""
    log_n, log_b, log_batch, K, coset, c = 10, 3, 7, 3, True, 8
    proofs = _prove(zk, log_n, log_b, log_batch, K, coset, c=c, q=q, g=g)
    _check_batch(zk, orc, proofs, log_n, log_b, K, coset, 0, 0, c, q, g)


# ---- 3. one live batch ------------------------------------------------------------------------------------------------------------------------
def test_one_live_batch_walked_through_ext_and_back(zk, orc):
    """ext 0 -> 1 -> 0 -> 1 -> 1 -> 0 -> 1 with K, leaf format, D and cap changing between the steps: stale planes, gather sizes, final
    tables or challenge rows would show.  The ext-off steps are byte-equal to a batch that never had ext on, and the device bytes with
    ext off are what they were before the first set_ext(1)."""
    import cap_ref
    log_n, log_b, log_batch, q = 5, 2, 3, 2
    nb, lib = 1 << log_batch, zk.load()
    walk = [(0, 1, False, 0, 0), (1, 3, True, 2, 3), (0, 2, True, 0, 8), (1, 1, False, 0, 0), (1, 2, False, 2, 8), (0, 3, False, 2, 0), (1, 3, True, 0, 3)]
    with zk.BatchContext(log_n, log_b, log_batch, queries=q) as bc, zk.BatchContext(log_n, log_b, log_batch, queries=q) as twin:
        # twin: the same walk on a batch that never has ext on -- the ext-off proofs and, with ext off, the device bytes of the walked batch
        bc.gen_fibsq(*_seeds(nb))
        twin.gen_fibsq(*_seeds(nb))
        base = None
        for ext, K, coset, D, c in walk:
            for b in (bc, twin):                             # the other settings change under whatever ext the walked batch has
                b.set_fold(K)
                b.set_coset_leaves(coset)
                b.set_fri_stop(D)
                b.set_merkle_cap(c)
            if ext and base is None:
                base = bc.device_bytes                       # before the first set_ext(1)
                assert base == twin.device_bytes
            bc.set_ext(ext)
            assert lib.zk_batch_get_ext(bc._h) == ext == bc.ext_log
            proofs = bc.prove()
            if ext:
                grown = bc.device_bytes
                assert grown > twin.device_bytes
                assert lib.zk_batch_set_ext(bc._h, 1) == 0 and bc.device_bytes == grown      # the value it has: nothing moves
                _check_batch(zk, orc, proofs, log_n, log_b, K, coset, 0, D, c, q, 0)
                _check_trees(zk, orc, bc, log_n, log_b, K, coset, 0, D, c, (0, nb - 1))
            else:
                assert bc.device_bytes == twin.device_bytes
                for p, (a, b) in enumerate(zip(proofs, twin.prove())):
                    assert a.ext_log == 0 and a.data == b.data and a.state == b.state
                    _same(a, cap_ref.proof(orc, log_n, log_b, q, 0, K, coset, D, c, 0, SEED + p))
        bc.set_ext(0)
        assert bc.device_bytes == twin.device_bytes
        for b in (bc, twin):                                 # back at the settings of the step before the first set_ext(1)
            b.set_fold(3); b.set_coset_leaves(True); b.set_fri_stop(2); b.set_merkle_cap(3)
        assert bc.device_bytes == twin.device_bytes == base


# ---- 4. a broken trace ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0, 2])
def test_a_broken_trace_names_its_proof(zk, orc, D):
    log_n, log_b, log_batch, bad = 6, 2, 3, 5
    n, nb = 1 << log_n, 1 << log_batch
    good = np.stack([_trace(zk, log_n, SEED + p) for p in range(nb)])
    broken = good.copy()
    broken[bad, 20] = (int(broken[bad, 20]) + 1) % P
    with zk.BatchContext(log_n, log_b, log_batch, queries=2, stop_log=D, ext_log=1) as bc:
        bc.set_traces(broken)
        with pytest.raises(zk.ZkError, match=f"proof {bad} of the batch") as e:
            bc.prove()
        assert e.value.code == ERR_CHECK
        bc.set_traces(good)
        proofs = bc.prove()
    _check_batch(zk, orc, proofs, log_n, log_b, 1, False, 0, D, 0, 2, 0)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_batch_ext_refusals(zk, orc):
    import shared_ref
    lib = zk.load()
    log_n, log_b, log_batch = 5, 2, 2
    with zk.BatchContext(log_n, log_b, log_batch, queries=2) as bc:
        assert lib.zk_batch_set_ext(bc._h, 2) == ERR_INVALID
        assert b"zk_batch_set_ext: ext_log must be 0 or 1 (got 2; 2, the quartic extension, is reserved)" in lib.zk_last_error()
        assert lib.zk_batch_get_ext(bc._h) == 0
        bc.gen_fibsq(*_seeds(bc.batch))
        bc.set_ext(1)
        with pytest.raises(zk.ZkError, match="zk_batch_prove_shared: the batch has ext_log = 1") as e:
            bc.prove_shared()
        assert e.value.code == ERR_STATE
        proofs = bc.prove()                                  # the batch keeps proving
        _check_batch(zk, orc, proofs, log_n, log_b, 1, False, 0, 0, 0, 2, 0)
        bc.set_ext(0)
        sp = bc.prove_shared()
        ref = shared_ref.proof(orc, log_n, log_b, log_batch, 2, 0, 1, False, 0, 0, 0)
        assert sp.data == ref.data and sp.state == ref.state and sp.check(strict=True) == 0
    with zk.BatchContext(6, 2, 0) as one:                    # a batch of one: through the forward
        assert lib.zk_batch_set_ext(one._h, 2) == ERR_INVALID and lib.zk_batch_get_ext(one._h) == 0
        assert lib.zk_batch_set_ext(one._h, 1) == 0 and lib.zk_batch_get_ext(one._h) == 1


def test_set_ext_is_refused_while_a_prove_runs(zk):
    """The shape of test_set_fri_stop_is_refused_while_a_prove_runs: zk_batch_set_ext from a second thread answers ZK_ERR_STATE while a
    zk_batch_prove holds the batch, and the proofs of that run are unharmed."""
    lib = zk.load()
    log_n, log_b, log_batch = 16, 3, 4
    with zk.BatchContext(log_n, log_b, log_batch, ext_log=1) as bc:
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
            seen.append(lib.zk_batch_set_ext(bc._h, 1))     # the value it already has: accepted when idle, and changes nothing
        t.join()
        assert ERR_STATE in seen
        assert set(seen) <= {0, ERR_STATE}
        assert (out["last"] == first).all()
        assert lib.zk_batch_set_ext(bc._h, 1) == 0 and lib.zk_batch_get_ext(bc._h) == 1
        again, _ = bc.prove_raw()
        assert (again == first).all()
