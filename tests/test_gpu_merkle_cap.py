"""Merkle caps on the GPU (zk_ctx_set_merkle_cap): the one-call provers against the proofs tests/cap_ref.py builds
without the library -- bytes and final state -- and zk_verify_cap accepting them, at the smallest shapes at which each new path can go
wrong: trees smaller than the cap (the clamp), a hand-over at depth > 0 for every hash with the host's share above, at and absent
below it, every setting the cap combines with, the throughput launches, and one context whose cap changes from proof to proof."""
import ctypes as C

import numpy as np
import pytest

import cap_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field", 2: "blake2s"}
ZK_ERR_INVALID, ZK_ERR_STATE = -1, -4
PREFIX = b"merkle cap prefix"
A1, A2 = 3141592, 2718281


def _trace(n, a1=A1):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


def _assert_proof(zk, p, ref, log_n, log_b, h, q, g, K, coset, D, c, what):
    lib = zk.load()
    assert len(p.data) == len(ref.data), (what, len(p.data), len(ref.data))
    assert (p.data, p.state) == (ref.data, ref.state), what
    body = p.data
    assert len(body) == lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, c), what
    for state in (None, p.state):
        out = C.c_int32(1)
        assert lib.zk_verify_cap(body, len(body), state, log_n, log_b, p.public_last, h, q, g, K, int(coset), D, c, C.byref(out)) == 0, (what, out.value)
        assert out.value == 0
    assert p.cap_log == c and p.check(strict=True) == 0 and p.check() == 0, what


@pytest.mark.parametrize("c", [1, 3, 8])
@pytest.mark.parametrize("log_n,log_b", [(4, 1), (5, 2)])
def test_clamped_caps(zk, orc, log_n, log_b, c):
    """Every FRI tree here has lg - 1 < c somewhere: c_eff = lg - 1 leaves one inner level and one path digest."""
    assert any(lg - 1 < c for _, lg in cap_ref.trees(log_n, log_b, 1, False, 0)) or c == 1
    trace = _trace(1 << log_n)
    for h, K, coset, D, q in ((0, 1, False, 0, 2), (1, 2, True, 0, 1), (2, 1, False, 1, 2), (0, 3, True, 1, 3), (1, 1, False, 0, 1), (2, 2, True, 0, 2)):
        ref = cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c)
        with zk.Context(log_n, log_b, hash=HASH_NAMES[h], queries=q, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c) as ctx:
            assert zk.load().zk_ctx_get_merkle_cap(ctx._h) == c
            _assert_proof(zk, ctx.prove(trace), ref, log_n, log_b, h, q, 0, K, coset, D, c, f"h{h} K{K} coset{coset} D{D}")


@pytest.mark.parametrize("levels", [None, (0, 0)], ids=["host-default", "host-off"])
@pytest.mark.parametrize("h", [0, 1, 2], ids=["sha256", "field", "blake2s"])
@pytest.mark.parametrize("c", [2, 5, 8])
def test_hashes_and_host_levels(zk, orc, c, h, levels):
    """(10, 3): c = 8 is the default hand-over depth (the host hashes nothing), c = 5 lies below it (the host stops early), c = 2 further;
    with the host levels off, and for hashes 1 and 2 always, the device hands over at the cap itself."""
    log_n, log_b, q = 10, 3, 2
    ref = cap_ref.proof(orc, log_n, log_b, q, h, 1, False, 0, c)
    with zk.Context(log_n, log_b, hash=HASH_NAMES[h], queries=q, host_levels=levels, cap_log=c) as ctx:
        if levels is None:
            assert ctx.host_levels[0] == 8
        _assert_proof(zk, ctx.prove(_trace(1 << log_n)), ref, log_n, log_b, h, q, 0, 1, False, 0, c, f"c{c} h{h} {levels}")


@pytest.mark.parametrize("K,coset,D", [(3, True, 4), (1, False, 4), (2, False, 0)], ids=["K3-coset-D4", "K1-plain-D4", "K2-plain-D0"])
def test_settings(zk, orc, K, coset, D):
    """c = 4 with three queries and four bits of grinding: zk_prove, zk_prove_channel behind a prefix, zk_prove_many on two traces."""
    log_n, log_b, q, g, c = 10, 3, 3, 4, 4
    ref1 = cap_ref.proof(orc, log_n, log_b, q, 0, K, coset, D, c, g, A1)
    ref2 = cap_ref.proof(orc, log_n, log_b, q, 0, K, coset, D, c, g, A2)
    refp = cap_ref.proof(orc, log_n, log_b, q, 0, K, coset, D, c, g, A2, PREFIX)
    kw = dict(queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c)
    with zk.Context(log_n, log_b, **kw) as a, zk.Context(log_n, log_b, **kw) as b:
        _assert_proof(zk, a.prove(_trace(1 << log_n, A1)), ref1, log_n, log_b, 0, q, g, K, coset, D, c, "prove")
        b.trace_upload(_trace(1 << log_n, A2))
        ch = zk.Channel()
        ch.commit(PREFIX)
        pc = b.prove_channel(ch)
        assert (pc.data, pc.state) == (refp.data, refp.state) and pc.cap_log == c
        pm = zk.prove_many([a, b])
        _assert_proof(zk, pm[0], ref1, log_n, log_b, 0, q, g, K, coset, D, c, "many0")
        _assert_proof(zk, pm[1], ref2, log_n, log_b, 0, q, g, K, coset, D, c, "many1")


def test_throughput_launches_and_continuation(zk, orc):
    """(15, 3), c = 8, SHA-256, default switches: the trees above the latency switch take the throughput launches first."""
    log_n, log_b, q, c = 15, 3, 2, 8
    ref = cap_ref.proof(orc, log_n, log_b, q, 0, 1, False, 0, c)
    with zk.Context(log_n, log_b, queries=q, cap_log=c) as ctx:
        _assert_proof(zk, ctx.prove(_trace(1 << log_n)), ref, log_n, log_b, 0, q, 0, 1, False, 0, c, "2^18")


def test_one_live_context(zk, orc):
    """c = 0 -> 5 -> 0 -> 8 with alternating traces: nothing of an earlier proof above the cap leaks into a later one, and the cap-0
    proofs are the plain reference's."""
    log_n, log_b, q = 10, 3, 2
    with zk.Context(log_n, log_b, queries=q) as ctx:
        for i, c in enumerate((0, 5, 0, 8)):
            a1 = (A1, A2)[i & 1]
            ctx.set_merkle_cap(c)
            ref = cap_ref.proof(orc, log_n, log_b, q, 0, 1, False, 0, c, 0, a1)
            _assert_proof(zk, ctx.prove(_trace(1 << log_n, a1)), ref, log_n, log_b, 0, q, 0, 1, False, 0, c, f"step {i} c{c}")


def test_state_after_a_proof(zk, orc):
    """zk_ctx_merkle_cap is the reference's cap, roots[] is zero for a capped tree, nodes above the cap are refused, nodes from the cap
    down are the reference heap's; a stand-alone commitment afterwards builds the whole tree again."""
    log_n, log_b, c = 10, 3, 5
    lib = zk.load()
    ref = cap_ref.proof(orc, log_n, log_b, 1, 0, 1, False, 0, c)
    with zk.Context(log_n, log_b, cap_log=c) as ctx:
        ctx.prove(_trace(1 << log_n))
        info = ctx.last_transcript()
        for tid, lg in cap_ref.trees(log_n, log_b, 1, False, 0):
            ce = cap_ref.c_eff(c, lg)
            assert lib.zk_ctx_merkle_cap_log(ctx._h, tid) == ce
            assert ctx.merkle_cap(tid).tobytes() == ref.c.caps[tid], tid
            assert bytes(info.roots[tid]) == bytes(32)
            out = C.create_string_buffer(32)
            first = (1 << ce) - 1
            if first:
                assert lib.zk_merkle_node(ctx._h, tid, first - 1, out) == ZK_ERR_STATE
                assert lib.zk_merkle_node(ctx._h, tid, 0, out) == ZK_ERR_STATE
                one = np.zeros((2, 32), dtype=np.uint8)
                assert lib.zk_merkle_nodes(ctx._h, tid, first - 1, 2, one.ctypes.data_as(C.c_void_p)) == ZK_ERR_STATE
            heap = ref.c.trees[tid]
            got = ctx.merkle_nodes(tid, first, len(heap) - first)
            assert np.array_equal(got, heap[first:]), tid
            assert ctx.merkle_node(tid, first) == bytes(heap[first])
        small = np.zeros(32, dtype=np.uint8)
        assert lib.zk_ctx_merkle_cap(ctx._h, 0, small.ctypes.data_as(C.c_void_p), 32) != 0           # 32 * 2^5 bytes do not fit
        root = ctx.merkle_commit(0)                          # the stage-by-stage API ignores the setting
        assert bytes(root) == bytes(ref.c.trees[0][0]) and lib.zk_ctx_merkle_cap_log(ctx._h, 0) == 0
        assert ctx.merkle_node(0, 0) == bytes(ref.c.trees[0][0])


def test_refusals(zk):
    lib = zk.load()
    with zk.Context(4, 1) as ctx:
        assert lib.zk_ctx_set_merkle_cap(ctx._h, 9) == ZK_ERR_INVALID and lib.zk_ctx_get_merkle_cap(ctx._h) == 0
        assert lib.zk_ctx_set_merkle_cap(ctx._h, 8) == 0 and lib.zk_ctx_get_merkle_cap(ctx._h) == 8
        out = np.zeros(32, dtype=np.uint8)
        assert lib.zk_ctx_merkle_cap(ctx._h, 0, out.ctypes.data_as(C.c_void_p), 32) == ZK_ERR_STATE   # no proof made yet
