"""FRI folding factor 2^K in the batched prover (zk_batch_set_fold, zk_dev_fri_fold_multi_batch; DESIGN.md "Folding factor"): the
batched multi-fold kernel against `steps` oracle folds per proof, and zk_batch_prove against the proofs tests/fold_ref.py builds
without the library -- bytes, state, public input, every node of every committed tree -- and against the one-call prover."""
import ctypes as C

import numpy as np
import pytest

import fold_ref
from transforms_ref import P, rand_field, require_memory

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER, ERR_CHECK = -1, -4, -5, -7
BETAS = (0, 1, P - 1, P + 5, 2**32 - 1)                      # the last two: raw challenges >= P
SEED = 3141592


@pytest.fixture
def hb():
    from sharded_mirror import HipBackend
    b = HipBackend(0)
    yield b
    b.close()


def _rounds(log_n):
    """Every round for small domains, the ends and the middle for large ones."""
    return range(log_n) if log_n <= 7 else sorted({0, 1, 2, log_n // 2, log_n - 4, log_n - 3, log_n - 2, log_n - 1})


def _dev_fold_batch(hb, dom, layers, log_m, rnd, steps, betas, aligned):
    """zk_dev_fri_fold_multi_batch over the proof-major batch of `layers`; returns [batch][m >> steps]."""
    from zkstark_amd._lib import check
    nb, m, off = len(layers), 1 << log_m, 0 if aligned else 1
    src, dst = hb.empty(nb * m + off)[off:], hb.empty(nb * (m >> steps) + off)[off:]
    assert (src.data_ptr() % 16 == 0) == aligned and (dst.data_ptr() % 16 == 0) == aligned
    src.copy_(hb.upload(np.concatenate(layers)))
    beta, work = hb.upload(np.array(betas, dtype=np.uint32)), hb.empty(8 * nb)
    check(hb.lib.zk_dev_fri_fold_multi_batch(dom, src.data_ptr(), dst.data_ptr(), log_m, rnd, steps, beta.data_ptr(), work.data_ptr(), nb,
                                             hb._stream()))
    return hb.to_host(dst).reshape(nb, m >> steps)


def _dev_fold_one(hb, dom, layer, log_m, rnd, steps, beta):
    from zkstark_amd._lib import check
    src, dst = hb.upload(layer), hb.empty(len(layer) >> steps)
    check(hb.lib.zk_dev_fri_fold_multi(dom, src.data_ptr(), dst.data_ptr(), log_m, rnd, steps, beta, hb._stream()))
    return hb.to_host(dst)


# ---- 1. the kernel against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 5, 7, 10, 13, 16])
def test_dev_fold_multi_batch_matches_the_oracle_per_proof(orc, hb, log_n):
    """Every (log_b, round, steps) of the grid with batches of 1, 2, 5 and 8 different layers, each folded with its own challenge,
    on 16-byte aligned buffers (four outputs per lane) and one word past (one output per lane).  log_b 1 and 2 end in layers of 2
    and 4 values per proof.  A batch of one also equals zk_dev_fri_fold_multi."""
    case, seen = 0, set()
    for log_b in (1, 2, 3):
        L = log_n + log_b
        dom = hb.domain(log_n, log_b, 5)
        rng = np.random.default_rng(1000 * log_n + log_b)
        for rnd in _rounds(log_n):
            layers = [rand_field(rng, 1 << (L - rnd)) for _ in range(8)]
            layers[0][0] = layers[7][-1] = P - 1
            for steps in (1, 2, 3):
                if rnd + steps > log_n:
                    continue
                betas = [BETAS[(p + case) % len(BETAS)] if (p + case) % 2 == 0 else int(rng.integers(0, 2**32)) for p in range(8)]
                seen.update(betas)
                want = [fold_ref.fold_layer(orc, layers[p], log_n, log_b, rnd, steps, betas[p]) for p in range(8)]
                for nb in (1, 2, 5, 8):
                    o = case % (8 - nb + 1)                             # which proofs of the eight form this batch
                    for aligned in ((True, False) if L - rnd <= 14 else (bool((case + nb) & 1),)):
                        got = _dev_fold_batch(hb, dom, layers[o:o + nb], L - rnd, rnd, steps, betas[o:o + nb], aligned)
                        for p in range(nb):
                            assert np.array_equal(got[p], want[o + p]), (log_b, rnd, steps, nb, o, p, betas[o + p], aligned)
                    if nb == 1:
                        assert np.array_equal(_dev_fold_one(hb, dom, layers[o], L - rnd, rnd, steps, betas[o]), want[o])
                case += 1
    assert seen >= set(BETAS)


def test_dev_fold_multi_batch_every_special_beta(orc, hb):
    """One batch of five whose challenges are exactly 0, 1, P - 1, P + 5 and 2^32 - 1; then the same in another order."""
    log_n, log_b, rnd = 9, 3, 2
    dom = hb.domain(log_n, log_b, 5)
    rng = np.random.default_rng(5)
    layers = [rand_field(rng, 1 << (log_n + log_b - rnd)) for _ in BETAS]
    for betas in (list(BETAS), list(BETAS[::-1])):
        for steps in (1, 2, 3):
            for aligned in (True, False):
                got = _dev_fold_batch(hb, dom, layers, log_n + log_b - rnd, rnd, steps, betas, aligned)
                for p, beta in enumerate(betas):
                    assert np.array_equal(got[p], fold_ref.fold_layer(orc, layers[p], log_n, log_b, rnd, steps, beta)), (beta, steps, aligned)


# ---- 2. one big shape ------------------------------------------------------------------------------------------------------------
def test_dev_fold_multi_batch_four_layers_of_2e24(orc, hb):
    """Four layers of 2^24 values (layer 0 of a 2^24 domain) -> layer 3, in one pass."""
    log_n, log_b, nb = 21, 3, 4
    require_memory(4 * (4 << 26), 4 * (4 << 26))
    dom = hb.domain(log_n, log_b, 5, fold_only=True)
    rng = np.random.default_rng(24)
    layers = [rand_field(rng, 1 << 24) for _ in range(nb)]
    betas = [P + 77, 0, int(rng.integers(0, 2**32)), 2**32 - 1]
    got = _dev_fold_batch(hb, dom, layers, 24, 0, 3, betas, True)
    for p in range(nb):
        assert np.array_equal(got[p], fold_ref.fold_layer(orc, layers[p], log_n, log_b, 0, 3, betas[p])), p


# ---- 3. the batched prover equals the reference proofs ---------------------------------------------------------------------------
def _same(p, ref):
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _seeds(batch, first=SEED):
    return [1] * batch, [first + p for p in range(batch)]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b", [(4, 1), (5, 2), (10, 3), (13, 1), (13, 3)])
@pytest.mark.parametrize("K", [2, 3])
def test_batch_prover_equals_the_reference(zk, orc, K, log_n, log_b, hash_kind):
    """Proof p of every batch is the reference's proof of fibsq(1, 3141592 + p): bytes, state, public input; host tree tops on and
    off give the same bytes.  (4, 1) with K = 3 has a last group of one round and a last layer of 2 values."""
    made = {}                                                # (log_batch, q) -> proofs
    for log_batch in (1, 3, 5):
        for q in (1, 7):
            g = 12 if (log_n, log_b, q) == (10, 3, 7) else 0
            with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K) as bc:
                assert bc.fold_log == K and zk.load().zk_batch_get_fold(bc._h) == K
                bc.gen_fibsq(*_seeds(1 << log_batch))
                per_levels = []
                for on in (1, 0):
                    assert zk.load().zk_batch_set_host_levels(bc._h, on) == 0
                    per_levels.append(bc.prove())
                for a, b in zip(*per_levels):
                    assert a.data == b.data and a.state == b.state
                made[log_batch, q] = per_levels[0]
    for p in range(1 << 5):                                  # one reference per (p, q); the transcript prefix is shared by q = 1, 7
        for q in (1, 7):
            g = 12 if (log_n, log_b, q) == (10, 3, 7) else 0
            ref = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, g, a1=SEED + p)
            for log_batch in (1, 3, 5):
                if p < (1 << log_batch):
                    got = made[log_batch, q][p]
                    _same(got, ref)
                    assert got.fold_log == K and got.queries == q and got.grind_bits == g
            got = made[5, q][p]
            assert got.check(strict=True) == 0 and got.check() == 0
            assert fold_ref.verify(orc, got.data, got.state, log_n, log_b, got.public_last, hash_kind, q, g, K) == 0


# ---- 4. ... and the single prover ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,log_n,log_b", [(2, 10, 3), (3, 7, 2)])
def test_batch_prover_equals_the_single_prover(zk, K, log_n, log_b):
    """Traces handed over from the host; every proof equals Context(fold_log=K).prove of its trace.  log_batch 0 runs on the
    one-call prover itself (a batch of one)."""
    q = 3
    with zk.Context(log_n, log_b, queries=q, fold_log=K) as ctx:
        for log_batch in (0, 3, 4):
            traces = np.stack([zk.trace_fibsq((1 << log_n) - 1, 1, 5 + 31 * log_batch + p) for p in range(1 << log_batch)])
            with zk.BatchContext(log_n, log_b, log_batch, queries=q, fold_log=K) as bc:
                bc.set_traces(traces)
                proofs = bc.prove()
            assert len(proofs) == 1 << log_batch
            for p, got in enumerate(proofs):
                one = ctx.prove(traces[p])
                assert got.data == one.data and got.state == one.state and got.public_last == one.public_last
                assert got.fold_log == K and got.check(strict=True) == 0


# ---- 5. trees --------------------------------------------------------------------------------------------------------------------
def _subtree(heap, log_batch, p, log_m):
    """Proof p's tree (2 * 2^log_m - 1 nodes, heap order) out of the batch heap."""
    rows = [heap[(1 << (log_batch + d)) - 1 + (p << d):(1 << (log_batch + d)) - 1 + ((p + 1) << d)] for d in range(log_m + 1)]
    return np.concatenate(rows)


@pytest.mark.parametrize("hash_kind,log_n,log_b,log_batch", [(0, 5, 2, 3), (0, 10, 3, 2), (1, 7, 1, 2), (0, 13, 3, 1)])
@pytest.mark.parametrize("K", [2, 3])
def test_batch_trees_of_a_folded_proof(zk, orc, K, hash_kind, log_n, log_b, log_batch):
    """Every node of every committed tree, host-built levels included; an id the proof did not commit: ZK_ERR_STATE."""
    L = log_n + log_b
    with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[hash_kind], fold_log=K) as bc:
        bc.gen_fibsq(*_seeds(1 << log_batch))
        proofs = bc.prove()
        committed = {0, 1} | {1 + r0 + s for r0, s in fold_ref.groups(log_n, K)}
        heaps = {i: bc.merkle_nodes(i) for i in sorted(committed)}
        for i in range(log_n + 2):
            if i in committed:
                continue
            for call in (lambda: bc.merkle_nodes(i), lambda: bc.merkle_nodes(i, 0, 1)):
                with pytest.raises(zk.ZkError, match=f"tree {i} .*fold_log {K}") as e:
                    call()
                assert e.value.code == ERR_STATE
    assert len(committed) < log_n + 2
    for p in range(1 << log_batch):
        ref = fold_ref.fold_proof(orc, log_n, log_b, 1, hash_kind, K, a1=SEED + p)
        _same(proofs[p], ref)
        assert sorted(ref.c.trees) == sorted(committed)
        for i in sorted(committed):
            log_m = L if i == 0 else L - (i - 1)
            assert np.array_equal(heaps[i][(1 << log_batch) - 1 + p], ref.c.trees[i][0]), (p, i)
            assert np.array_equal(_subtree(heaps[i], log_batch, p, log_m), ref.c.trees[i]), (p, i)


# ---- 6. state across proofs ------------------------------------------------------------------------------------------------------
def test_one_batch_goes_from_factor_to_factor(zk, orc):
    log_n, log_b, log_batch, q = 7, 2, 2, 2
    A, B = _seeds(1 << log_batch), _seeds(1 << log_batch, 271828)
    with zk.BatchContext(log_n, log_b, log_batch, queries=q) as bc:
        for K, (a0s, a1s) in ((3, A), (1, B), (2, A)):
            bc.set_fold(K)
            bc.gen_fibsq(a0s, a1s)
            proofs = bc.prove()
            for p, got in enumerate(proofs):
                _same(got, fold_ref.fold_proof(orc, log_n, log_b, q, 0, K, a1=a1s[p]))
                assert got.fold_log == K and got.check(strict=True) == 0
            if K == 1:                                       # every id is materialised again
                for i in range(log_n + 2):
                    assert len(bc.merkle_nodes(i, 0, 1)) == 1
                one = fold_ref.fold_proof(orc, log_n, log_b, q, 0, 1, a1=a1s[1])
                assert bytes(bc.merkle_nodes(2, (1 << log_batch) - 1 + 1, 1)[0]) == one.c.roots[2]
            else:
                with pytest.raises(zk.ZkError) as e:
                    bc.merkle_nodes(2, 0, 1)
                assert e.value.code == ERR_STATE


# ---- 7. setter rules -------------------------------------------------------------------------------------------------------------
def test_set_fold_argument_and_buffer_errors(zk):
    lib = zk.load()
    log_n, log_b, log_batch = 8, 2, 2
    with zk.BatchContext(log_n, log_b, log_batch, queries=2, fold_log=2) as bc:
        for K in (0, 4):
            assert lib.zk_batch_set_fold(bc._h, K) == ERR_INVALID
            assert lib.zk_batch_get_fold(bc._h) == 2
        with pytest.raises(zk.ZkError):
            bc.set_fold(4)
        assert bc.fold_log == 2
        traces = np.stack([zk.trace_fibsq((1 << log_n) - 1, 1, 9 + p) for p in range(1 << log_batch)])
        bc.set_traces(traces)
        plen = lib.zk_proof_data_len_fold(log_n, log_b, 2, 0, 2)
        assert plen != lib.zk_proof_data_len_queries(log_n, log_b, 2)
        data = np.zeros((bc.batch, plen), dtype=np.uint8)
        states = np.zeros((bc.batch, 32), dtype=np.uint8)
        rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen - 1, states.ctypes.data_as(C.c_void_p))
        assert rc == ERR_BUFFER and str(plen).encode() in lib.zk_last_error()
        assert lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p)) == 0
        assert (data == bc.prove_raw()[0]).all()
        traces[2, 100] = (int(traces[2, 100]) + 1) % P      # a broken trace in one proof of a folded batch
        bc.set_traces(traces)
        with pytest.raises(zk.ZkError, match="proof 2") as e:
            bc.prove()
        assert e.value.code == ERR_CHECK
    with zk.BatchContext(log_n, log_b, 0, fold_log=3) as one:   # a batch of one forwards to its context
        for K in (0, 4):
            assert lib.zk_batch_set_fold(one._h, K) == ERR_INVALID
        assert lib.zk_batch_get_fold(one._h) == 3


def test_set_fold_is_refused_while_a_prove_runs(zk):
    """The shape of test_batch_setters_are_refused_while_a_prove_runs: zk_batch_set_fold from a second thread answers ZK_ERR_STATE
    while a zk_batch_prove holds the batch, and the proofs of that run are unharmed."""
    import threading
    lib = zk.load()
    log_n, log_b, log_batch, K = 16, 3, 4, 2
    with zk.BatchContext(log_n, log_b, log_batch, fold_log=K) as bc:
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
            seen.append(lib.zk_batch_set_fold(bc._h, K))    # the factor it already has: accepted when idle, and changes nothing
        t.join()
        assert ERR_STATE in seen
        assert set(seen) <= {0, ERR_STATE}
        assert (out["last"] == first).all()
        assert lib.zk_batch_set_fold(bc._h, K) == 0 and lib.zk_batch_get_fold(bc._h) == K
        again, _ = bc.prove_raw()
        assert (again == first).all()


# ---- 8. domain 2^24 --------------------------------------------------------------------------------------------------------------
def test_batch_domain_2e24(zk, orc):
    """Two 2^24 proofs in lockstep, K = 3, SHA-256: proof 0 is the reference's, proof 1 the one-call prover's of the same trace,
    and the strict verifier accepts both."""
    log_n, log_b, K = 21, 3, 3
    require_memory(10 << 30, 6 << 30)
    seeds = [SEED, SEED + 1]
    with zk.BatchContext(log_n, log_b, 1, fold_log=K) as bc:
        bc.gen_fibsq([1, 1], seeds)
        proofs = bc.prove()
    ref = fold_ref.fold_proof(orc, log_n, log_b, 1, 0, K)
    fold_ref.committed.cache_clear()
    _same(proofs[0], ref)
    with zk.Context(log_n, log_b, fold_log=K) as ctx:
        one = ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, seeds[1]))
    assert proofs[1].data == one.data and proofs[1].state == one.state and proofs[1].public_last == one.public_last
    for p in proofs:
        out = C.c_int32(7)
        assert zk.load().zk_verify_fold(p.data, len(p.data), p.state, log_n, log_b, p.public_last, 0, 1, 0, K, C.byref(out)) == 0 and out.value == 0
