"""Merkle caps in the batched prover (zk_batch_set_merkle_cap): zk_batch_prove against the proofs tests/cap_ref.py
builds without the library -- bytes, state, public input -- and against the one-call prover with the same cap, at the smallest shapes
that reach each way a capped batch tree gets to the host: the mailbox at the cap's depth, the mailbox with host levels above the cap,
and, for caps the mailbox cannot hold, a build that ends at the cap (below, at and above the latency switch F = 17) followed by
digest_level_post_kernel.  H: heap depth of the f tree, e = log_batch + ce: the depth of its cap in the batch heap."""
import ctypes as C

import numpy as np
import pytest

import cap_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER = -1, -4, -5
SEED = 3141592


def _same(p, ref):
    assert len(p.data) == len(ref.data), (len(p.data), len(ref.data))
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _seeds(batch, first=SEED):
    return [1] * batch, [first + p for p in range(batch)]


def _trace(zk, log_n, a1):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


def _check_batch(zk, orc, proofs, log_n, log_b, c, K, coset, h, D, q, g, first=SEED):
    """Every proof: the one-call prover's with the same settings, the length the format gives, accepted by the strict CPU verifier.
    The Python reference: every proof of a batch of <= 32, else the first and the last."""
    lib, nb = zk.load(), len(proofs)
    plen = lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, c)
    assert plen == cap_ref.proof_len(log_n, log_b, q, g, K, coset, D, c)
    with zk.Context(log_n, log_b, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c) as ctx:
        for p, got in enumerate(proofs):
            _same(got, ctx.prove(_trace(zk, log_n, first + p)))
    for p in (range(nb) if nb <= 32 else (0, nb - 1)):
        _same(proofs[p], cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, g, first + p))
    for got in proofs:
        assert len(got.data) == plen and got.cap_log == c
        assert (got.fold_log, got.queries, got.grind_bits, got.coset_leaves, got.stop_log) == (K, q, g, coset, D)
        assert got.check(strict=True) == 0


def _prove(zk, log_n, log_b, log_batch, c, K=1, coset=False, h=0, D=0, q=2, g=0, levels=(None,)):
    """The proofs of fibsq(1, SEED + p); levels: the host-levels settings to run (None: the default), whose bytes must agree."""
    lib = zk.load()
    with zk.BatchContext(log_n, log_b, log_batch, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D,
                         cap_log=c) as bc:
        assert bc.cap_log == c and lib.zk_batch_get_merkle_cap(bc._h) == c
        assert bc.proof_len == lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, c)
        bc.gen_fibsq(*_seeds(1 << log_batch))
        runs = []
        for on in levels:
            if on is not None:
                assert lib.zk_batch_set_host_levels(bc._h, on) == 0
            runs.append(bc.prove())
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.data == b.data and a.state == b.state
        if log_batch:
            for tid, lg in cap_ref.trees(log_n, log_b, K, coset, D):
                assert lib.zk_batch_merkle_cap_log(bc._h, tid) == cap_ref.c_eff(c, lg), tid
    return runs[0]


# ---- 1. the shapes --------------------------------------------------------------------------------------------------------------------
# (log_n, log_b, log_batch, c):
#   (4, 1, 1, 8)    every tree's cap is clamped to lg - 1: paths of one digest or none; mailbox
#   (5, 2, 5, 1)    host levels h = 5 above ce = 1: the host hashes from 5 down to 1
#   (5, 2, 5, 3)    ... down to 3
#   (5, 2, 5, 8)    e = 11 > 10, H = 12 <= F: the post kernel behind a latency-only build; the small FRI trees take the mailbox
#   (10, 3, 7, 8)   H = 20 > F > e = 15: throughput launches, a latency phase that ends at 2^15 nodes, the post
#   (10, 3, 7, 2)   e = 9: mailbox, the host hashes one level
#   (7, 2, 9, 8)    e = 17 = F < H = 18: one throughput launch and no latency phase
#   (7, 2, 10, 8)   e = 18 > F, H = 19: throughput only, 2^18 digests posted
#   (6, 2, 0, 5)    the batch of one forwards to its context
SHAPES = [(4, 1, 1, 8), (5, 2, 5, 1), (5, 2, 5, 3), (5, 2, 5, 8), (10, 3, 7, 8), (10, 3, 7, 2), (7, 2, 9, 8), (7, 2, 10, 8), (6, 2, 0, 5)]


@pytest.mark.parametrize("K,coset", [(1, False), (3, True)], ids=["K1-plain", "K3-coset"])
@pytest.mark.parametrize("log_n,log_b,log_batch,c", SHAPES, ids=["clamped", "host-5-to-1", "host-5-to-3", "post-latency-only", "post-after-latency",
                                                                 "mailbox-one-host-level", "post-at-the-switch", "post-throughput-only", "batch-of-one"])
def test_batch_cap_shapes(zk, orc, log_n, log_b, log_batch, c, K, coset):
    levels = (1, 0) if 0 < log_batch <= 5 else (None,)
    proofs = _prove(zk, log_n, log_b, log_batch, c, K, coset, levels=levels)
    assert len(proofs) == 1 << log_batch
    _check_batch(zk, orc, proofs, log_n, log_b, c, K, coset, 0, 0, 2, 0)


def test_batch_cap_queries_and_grinding(zk, orc):
    """q = 7 and 12 bits of grinding on the shape whose f cap goes through the post kernel behind both kinds of launches."""
    log_n, log_b, log_batch, c, K, coset, q, g = 10, 3, 7, 8, 3, True, 7, 12
    proofs = _prove(zk, log_n, log_b, log_batch, c, K, coset, q=q, g=g)
    _check_batch(zk, orc, proofs, log_n, log_b, c, K, coset, 0, 0, q, g)


# ---- 2. every setting the cap combines with ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [0, 2])
@pytest.mark.parametrize("h", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("c", [3, 8])
def test_batch_cap_crossings(zk, orc, c, K, coset, h, D):
    log_n, log_b, log_batch = 5, 2, 5
    proofs = _prove(zk, log_n, log_b, log_batch, c, K, coset, h, D, levels=(1, 0))
    _check_batch(zk, orc, proofs, log_n, log_b, c, K, coset, h, D, 2, 0)


# ---- 3. the trees after a proof -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_b,log_batch,c", [(5, 2, 5, 8), (7, 2, 9, 8)], ids=["latency-only", "at-the-switch"])
def test_batch_cap_tree_read_out(zk, orc, log_n, log_b, log_batch, c):
    """Tree 0 does not depend on c: from the cap's depth down it is the heap of a cap-0 run; one index above the cap is refused;
    merkle_cap(t, p) is the reference's cap of every tree the proof built."""
    lib, nb, L = zk.load(), 1 << log_batch, log_n + log_b
    ce = cap_ref.c_eff(c, L)
    first = (1 << (log_batch + ce)) - 1
    with zk.BatchContext(log_n, log_b, log_batch, queries=2) as bc:
        bc.gen_fibsq(*_seeds(nb))
        bc.prove()
        want = bc.merkle_nodes(0, first)
        assert len(want) == 2 * nb * (1 << L) - 1 - first
        bc.set_merkle_cap(c)
        bc.prove()
        assert lib.zk_batch_merkle_cap_log(bc._h, 0) == ce
        got = bc.merkle_nodes(0, first)
        assert np.array_equal(got, want)
        out = np.zeros((2, 32), dtype=np.uint8)
        for idx, cnt in ((first - 1, 1), (first - 1, 2), (0, 1)):
            assert lib.zk_batch_merkle_nodes(bc._h, 0, idx, cnt, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
            assert b"lies above its Merkle cap" in lib.zk_last_error()
        assert lib.zk_batch_merkle_nodes(bc._h, 0, first, 2, out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(out, want[:2])
        for p in (0, nb - 1):
            cm = cap_ref.committed(orc, log_n, log_b, 0, 1, False, 0, c, SEED + p)
            for tid, lg in cap_ref.trees(log_n, log_b, 1, False, 0):
                assert bc.merkle_cap(tid, p).tobytes() == cm.caps[tid], (p, tid)
        small = np.zeros(32, dtype=np.uint8)
        assert lib.zk_batch_merkle_cap(bc._h, 0, 0, small.ctypes.data_as(C.c_void_p), 32) == ERR_BUFFER
        assert lib.zk_batch_merkle_cap(bc._h, 0, nb, small.ctypes.data_as(C.c_void_p), 32) == ERR_INVALID


# ---- 4. one live batch ----------------------------------------------------------------------------------------------------------------------
def test_one_batch_goes_through_caps(zk, orc):
    """c = 0 -> 8 -> 3 -> 0 with the folding factor changed on the way: stale gather sizes, a stale tree_cap or a pinned buffer kept
    or lost would show.  (5, 2, 5): c = 8 needs the pinned buffer (e = 11), c = 3 gives it back."""
    log_n, log_b, log_batch, q = 5, 2, 5, 2
    nb, lib = 1 << log_batch, zk.load()
    A, B = _seeds(nb), _seeds(nb, 271828)
    walk = ((0, 2, A), (8, 2, B), (3, 1, A), (0, 1, B))
    fresh = {}
    for c, K, seeds in walk:
        if c == 0:
            with zk.BatchContext(log_n, log_b, log_batch, queries=q, fold_log=K) as f:
                f.gen_fibsq(*seeds)
                fresh[K] = f.prove()
    with zk.BatchContext(log_n, log_b, log_batch, queries=q, fold_log=2) as bc:
        bytes0 = bc.device_bytes                             # the multi-fold's work buffer, which is never given back, included
        for c, K, seeds in walk:
            bc.set_fold(K)
            bc.set_merkle_cap(c)
            assert lib.zk_batch_get_merkle_cap(bc._h) == c == bc.cap_log and lib.zk_batch_get_fold(bc._h) == K
            assert (bc.device_bytes > bytes0) == (c == 8), (c, bc.device_bytes, bytes0)
            bc.gen_fibsq(*seeds)
            proofs = bc.prove()
            _check_batch(zk, orc, proofs, log_n, log_b, c, K, False, 0, 0, q, 0, first=seeds[1][0])
            if c == 0:
                for a, b in zip(proofs, fresh[K]):
                    assert a.data == b.data and a.state == b.state
        assert bc.device_bytes == bytes0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_batch_cap_refusals(zk):
    lib = zk.load()
    log_n, log_b, log_batch, c = 5, 2, 2, 4
    with zk.BatchContext(log_n, log_b, log_batch, cap_log=c) as bc:
        assert lib.zk_batch_set_merkle_cap(bc._h, 9) == ERR_INVALID
        assert b"zk_batch_set_merkle_cap: need cap_log <= 8" in lib.zk_last_error()
        assert lib.zk_batch_get_merkle_cap(bc._h) == c
        small = np.zeros(32, dtype=np.uint8)
        assert lib.zk_batch_merkle_cap(bc._h, 0, 0, small.ctypes.data_as(C.c_void_p), 32) == ERR_STATE     # no proof made yet
        bc.gen_fibsq(*_seeds(bc.batch))
        plen = bc.proof_len
        assert plen == lib.zk_proof_data_len_cap(log_n, log_b, 1, 0, 1, 0, 0, c) != lib.zk_proof_data_len_fold(log_n, log_b, 1, 0, 1)
        data = np.zeros((bc.batch, plen), dtype=np.uint8)
        states = np.zeros((bc.batch, 32), dtype=np.uint8)
        rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen - 1, states.ctypes.data_as(C.c_void_p))
        assert rc == ERR_BUFFER and str(plen).encode() in lib.zk_last_error()
        assert lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p)) == 0
        assert lib.zk_batch_set_hash(bc._h, 2) == ERR_INVALID
    with pytest.raises(ValueError, match="hash='blake2s' is not built for this class yet"):
        zk.BatchContext(log_n, log_b, log_batch, hash="blake2s", cap_log=c)
    with zk.BatchContext(6, 2, 0) as one:                    # a batch of one: through the forward
        assert lib.zk_batch_set_merkle_cap(one._h, 9) == ERR_INVALID and lib.zk_batch_get_merkle_cap(one._h) == 0
        assert lib.zk_batch_set_merkle_cap(one._h, 5) == 0 and lib.zk_batch_get_merkle_cap(one._h) == 5


# ---- 6. made by the batch, checked by the GPU verifier ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_b,log_batch,c", [(5, 2, 5, 8), (10, 3, 7, 8)], ids=["latency-only", "after-latency"])
def test_batch_cap_proofs_pass_the_gpu_verifier(zk, log_n, log_b, log_batch, c):
    """Verifier(cap_log=c) accepts the whole batch; with one byte flipped inside a cap digest of proof p it rejects p alone, with the
    number zk_verify_cap gives on the CPU."""
    q, nb = 2, 1 << log_batch
    proofs = _prove(zk, log_n, log_b, log_batch, c, q=q)
    bad_p = nb - 3
    bad = bytearray(proofs[bad_p].data)
    bad[32 + 5] ^= 0x10                                      # inside the second digest of the f cap
    broken = list(proofs)
    broken[bad_p] = zk.Proof(proofs[bad_p].state, bytes(bad), log_n, log_b, proofs[bad_p].public_last, "sha256", q, 0, 1, False, 0, c)
    with zk.Verifier(log_n, log_b, queries=q, cap_log=c) as v:
        for strict in (True, False):
            got = v.verify(proofs, strict=strict)
            assert len(got) == nb and not got.any(), got
            got = v.verify(broken, strict=strict)
            want = broken[bad_p].check(strict=strict)       # not strict: 0 unless a path lands in the changed entry
            assert (want != 0 or not strict) and got[bad_p] == want, (got[bad_p], want)
            assert not np.delete(got, bad_p).any(), got
