"""The shared proof of the batched prover (zk_batch_prove_shared) on the GPU: byte equality with the model tests/shared_ref.py
builds without the library -- proof, state, public inputs -- at the smallest shapes that reach every path of compose_sum_batch_kernel and
of the stages run one proof wide, crossed with every setting; one live batch that alternates zk_batch_prove and zk_batch_prove_shared;
a broken trace; the refusals."""
import ctypes as C
import threading

import numpy as np
import pytest

import cap_ref
import shared_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER, ERR_CHECK = -1, -4, -5, -7
SEED = shared_ref.SEED


def _seeds(batch):
    return [1] * batch, [SEED + p for p in range(batch)]


def _same(got, ref, lib, s):
    log_n, log_b, lb, K, coset, D, c, q, g, h = s
    assert len(got.data) == len(ref.data) == lib.zk_proof_data_len_shared(log_n, log_b, q, g, K, int(coset), D, c, lb) == got.expected_len()
    assert got.data == ref.data, "proof bytes"
    assert got.state == ref.state and list(got.public_last) == list(ref.public_last)
    assert got.check(strict=True) == 0 and got.check() == 0
    got.verify(strict=True)


# (log_n, log_b, lb, K, coset, D, c, q, grind, hash), host levels to run (None: the default), whose bytes must agree
#   (2,1,1)      N = 8: one value per thread, B = 2
#   (4,1,*)      B = 2: the windows of two vectors, four values per thread
#   (5,2,3)      B = 4: whole vectors; a wave of the f build spans statements
#   (5,2,2) g 12 the nonce is searched on the device (above kGrindHostMaxBits = 10) with one job
#   (7,2,2) c 8  the caps clamp on the small FRI trees, the f level is 2^10 digests through the mailbox
#   (7,2,4) c 8  the f level is 2^12 digests through the post kernel
#   (6,2,8)      256 statements
#   (10,3,3)     the host's share of the tree tops at both widths, the fused fold at K = 1
CASES = [
    ((2, 1, 1, 1, False, 0, 0, 1, 0, 0), (None,)),
    ((2, 1, 1, 2, True, 0, 0, 1, 0, 1), (None,)),
    ((4, 1, 1, 1, False, 0, 0, 2, 0, 0), (1,)),
    ((4, 1, 1, 2, True, 2, 8, 2, 0, 0), (0,)),
    ((4, 1, 3, 3, False, 0, 3, 1, 0, 1), (None,)),
    ((4, 1, 3, 1, True, 0, 0, 16, 0, 0), (None,)),
    ((5, 2, 3, 1, False, 0, 0, 1, 8, 0), (None,)),
    ((5, 2, 2, 1, False, 0, 0, 1, 12, 0), (None,)),
    ((5, 2, 3, 3, True, 2, 3, 3, 0, 1), (None,)),
    ((5, 2, 3, 2, False, 2, 8, 2, 0, 0), (1, 0)),
    ((7, 2, 2, 1, False, 0, 8, 2, 0, 0), (1, 0)),
    ((7, 2, 2, 3, True, 0, 8, 2, 0, 0), (0,)),
    ((7, 2, 2, 2, False, 2, 8, 1, 0, 1), (None,)),
    ((7, 2, 4, 1, False, 0, 8, 2, 0, 0), (None,)),
    ((7, 2, 4, 3, True, 2, 8, 16, 0, 0), (None,)),
    ((7, 2, 4, 2, True, 0, 8, 1, 8, 1), (None,)),
    ((6, 2, 8, 1, False, 0, 0, 1, 0, 0), (None,)),
    ((6, 2, 8, 3, True, 2, 3, 2, 0, 0), (None,)),
    ((6, 2, 8, 2, False, 0, 3, 1, 0, 1), (None,)),
    ((10, 3, 3, 1, False, 0, 0, 1, 0, 0), (1, 0)),
    ((10, 3, 3, 3, True, 2, 3, 2, 8, 0), (1,)),
    ((10, 3, 3, 2, False, 0, 8, 16, 0, 1), (None,)),
    ((10, 3, 3, 1, True, 2, 0, 1, 0, 0), (0,)),
    ((10, 3, 3, 3, False, 0, 3, 2, 0, 0), (1, 0)),
]


def test_every_setting_appears():
    col = list(zip(*[s for s, _ in CASES]))
    assert set(col[3]) == {1, 2, 3} and set(col[4]) == {False, True} and set(col[5]) == {0, 2} and set(col[6]) == {0, 3, 8}
    assert {1, 16} <= set(col[7]) and set(col[8]) == {0, 8, 12} and set(col[9]) == {0, 1}
    assert {lv for _, levels in CASES for lv in levels} == {None, 0, 1}


@pytest.mark.parametrize("s,levels", CASES, ids=lambda v: "-".join(str(int(x)) if x is not None else "d" for x in v))
def test_shared_proof_is_the_model(zk, orc, s, levels):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, g, h = s
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, g)
    with zk.BatchContext(log_n, log_b, lb, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c) as bc:
        bc.gen_fibsq(*_seeds(1 << lb))
        for on in levels:
            if on is not None:
                assert lib.zk_batch_set_host_levels(bc._h, on) == 0
            _same(bc.prove_shared(), ref, lib, s)
        # tree 0 is the batch's f heap as ever: statement p's committed digests are the model's
        for p in {0, (1 << lb) - 1}:
            assert bc.merkle_cap(0, p).tobytes() == cap_ref.cap_of(ref.c.f_trees[p], ref.c.ce[0])
        out = np.zeros(32, dtype=np.uint8)
        assert lib.zk_batch_merkle_nodes(bc._h, 1, 0, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE


def test_live_batch_alternates_both_provers(zk, orc):
    """prove, prove_shared, K = 3 + coset leaves, prove_shared, prove on one batch: every zk_batch_prove proof is the one-call prover's,
    every shared proof the model's, and after a shared proof tree 0 is readable while tree 1 answers ZK_ERR_STATE."""
    lib = zk.load()
    log_n, log_b, lb, q = 7, 2, 2, 2
    nb = 1 << lb
    out = np.zeros(32, dtype=np.uint8)

    def plain_ok(bc, K, coset):
        got = bc.prove()
        with zk.Context(log_n, log_b, queries=q, fold_log=K, coset_leaves=coset) as ctx:
            for p in range(nb):
                want = ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, SEED + p))
                assert got[p].data == want.data and got[p].state == want.state and got[p].public_last == want.public_last
        assert lib.zk_batch_merkle_nodes(bc._h, 1, 0, 1, out.ctypes.data_as(C.c_void_p)) == 0

    def shared_ok(bc, K, coset):
        s = (log_n, log_b, lb, K, coset, 0, 0, q, 0, 0)
        ref = shared_ref.proof(orc, log_n, log_b, lb, q, 0, K, coset, 0, 0)
        _same(bc.prove_shared(), ref, lib, s)
        heap = bc.merkle_nodes(0, (1 << lb) - 1, nb)         # the per-statement roots of the f heap
        assert heap.tobytes() == b"".join(bytes(t[0]) for t in ref.c.f_trees)
        assert lib.zk_batch_merkle_nodes(bc._h, 1, 0, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert lib.zk_batch_merkle_cap(bc._h, 1, 0, out.ctypes.data_as(C.c_void_p), 32) == ERR_STATE

    with zk.BatchContext(log_n, log_b, lb, queries=q) as bc:
        before = bc.device_bytes
        bc.gen_fibsq(*_seeds(nb))
        plain_ok(bc, 1, False)
        shared_ok(bc, 1, False)
        assert bc.device_bytes == before                    # the shared proof allocates nothing on the device
        bc.set_fold(3)
        bc.set_coset_leaves(True)
        shared_ok(bc, 3, True)
        plain_ok(bc, 3, True)


def test_a_broken_trace_fails_the_batch_check(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, q = 5, 2, 2, 1
    nb, n = 1 << lb, 1 << log_n
    good = np.stack([zk.trace_fibsq(n - 1, 1, SEED + p) for p in range(nb)]).astype(np.uint32)
    bad = good.copy()
    bad[2, 11] = (int(bad[2, 11]) + 1) % shared_ref.P
    for K, coset, D in ((1, False, 0), (2, True, 2)):
        with zk.BatchContext(log_n, log_b, lb, queries=q, fold_log=K, coset_leaves=coset, stop_log=D) as bc:
            bc.set_traces(bad)
            with pytest.raises(zk.ZkError) as e:
                bc.prove_shared()
            assert e.value.code == ERR_CHECK and "some trace of the batch" in str(e.value)
            bc.set_traces(good)
            _same(bc.prove_shared(), shared_ref.proof(orc, log_n, log_b, lb, q, 0, K, coset, D, 0), lib, (log_n, log_b, lb, K, coset, D, 0, q, 0, 0))


def test_refusals(zk, orc):
    lib = zk.load()
    state, got = np.zeros(32, dtype=np.uint8), C.c_size_t(0)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for lb in (0, 9):                                        # a batch of one is a plain proof; 2^9 statements are too many
        with zk.BatchContext(4, 1, lb) as bc:
            bc.gen_fibsq(*_seeds(1 << lb))
            assert lib.zk_batch_prove_shared(bc._h, ptr(buf), buf.size, C.byref(got), ptr(state)) == ERR_INVALID
            assert "log_batch" in lib.zk_last_error().decode()
            with pytest.raises(zk.ZkError):
                bc.prove_shared()
    with zk.BatchContext(4, 1, 2) as bc:
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), buf.size, C.byref(got), ptr(state)) == ERR_STATE   # no traces
        bc.gen_fibsq(*_seeds(4))
        want = lib.zk_proof_data_len_shared(4, 1, 1, 0, 1, 0, 0, 0, 2)
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), want - 1, C.byref(got), ptr(state)) == ERR_BUFFER
        assert got.value == want and str(want) in lib.zk_last_error().decode()
        assert lib.zk_batch_prove_shared(bc._h, None, want, C.byref(got), ptr(state)) == ERR_INVALID
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), want, C.byref(got), ptr(state)) == 0
        assert buf[:want].tobytes() == shared_ref.proof(orc, 4, 1, 2, 1, 0, 1, False, 0, 0).data


def test_a_second_prove_on_a_busy_batch_is_refused(zk, orc):
    """zk_batch_prove on one thread, zk_batch_prove_shared on another: each shared call either is refused with ZK_ERR_STATE or gives
    the model's proof, and the plain proofs are never disturbed."""
    lib = zk.load()
    log_n, log_b, lb = 10, 3, 3
    ref = shared_ref.proof(orc, log_n, log_b, lb, 1, 0, 1, False, 0, 0)
    with zk.BatchContext(log_n, log_b, lb) as bc:
        bc.gen_fibsq(*_seeds(1 << lb))
        first = bc.prove_raw()
        plain, errors = [], []

        def run():
            try:
                for _ in range(6):
                    plain.append(bc.prove_raw())
            except zk.ZkError as e:                          # the shared call held the batch: refused, not disturbed
                errors.append(e.code)

        t = threading.Thread(target=run)
        t.start()
        codes = []
        while t.is_alive() and len(codes) < 50:
            try:
                got = bc.prove_shared()
                assert got.data == ref.data and got.state == ref.state
                codes.append(0)
            except zk.ZkError as e:
                codes.append(e.code)
        t.join()
        assert set(codes) <= {0, ERR_STATE} and set(errors) <= {ERR_STATE}, (codes, errors)
        for data, states in plain:
            assert np.array_equal(data, first[0]) and np.array_equal(states, first[1])
