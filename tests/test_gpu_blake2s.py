"""BLAKE2s-256 as a Merkle hash on the GPU (ZK_HASH_BLAKE2S): every node of trees built by the latency kernel alone and
by b2s_subtree_kernel in both modes and at every k, against hashlib.blake2s; whole proofs of the one-call provers against
tests/blake2s_ref.py, byte for byte with the final state and every committed tree -- up to 2^17-leaf trees, with the switch lowered so
that the fused leaf sources run at every k, and with early launch; one live context walked through the three hashes; and the entry
points that refuse the hash.  Equality everywhere.  (Every launch plan, node for node: tests/test_gpu_merkle_plans.py.)"""
import ctypes as C
import functools

import numpy as np
import pytest

import blake2s_ref
import stop_ref

pytestmark = pytest.mark.gpu

KIND = blake2s_ref.HASH_KIND
PREFIX = b"blake2s prefix"
ZK_ERR_INVALID = -1


def _trace(n, a1=3141592):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


@functools.lru_cache(maxsize=None)
def _leaves():
    """2^17 random words, 0 and 0xffffffff among the first two (so in every tree below); a tree of m leaves takes the first m."""
    v = np.random.default_rng(2).integers(0, 1 << 32, 1 << 17, dtype=np.uint64).astype(np.uint32)
    v[0], v[1] = 0, 0xFFFFFFFF
    return v


@functools.lru_cache(maxsize=None)
def _ref_tree(m):
    return blake2s_ref.tree(_leaves()[:m])


def _assert_nodes(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} nodes differ; first at heap indices {list(bad[:6])}"


class _latency_log:
    """zk_dev_set_merkle_latency_log for one case (process-wide), restored to the default on the way out."""

    def __init__(self, lib, lat):
        self.lib, self.lat = lib, lat

    def __enter__(self):
        assert self.lib.zk_dev_set_merkle_latency_log(self.lat) == 0

    def __exit__(self, *exc):
        assert self.lib.zk_dev_set_merkle_latency_log(0) == 0


# ---- trees ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 4, 64, 128, 1 << 10, 1 << 11, 1 << 13])
def test_trees_of_the_latency_kernel(zk, m):
    """The default switch (2^17 nodes): merkle_wg_kernel<PlainSrc, *, 2> alone -- one launch up to 2^10 leaves, two from 2^11 on (leaf
    mode, then inner mode)."""
    t = zk.Merkle(m, _leaves()[:m], hash="blake2s")
    _assert_nodes(t.nodes, _ref_tree(m), f"2^{m.bit_length() - 1} leaves")
    assert t.trace(m - 1) == blake2s_ref.path(_ref_tree(m), m - 1)


@pytest.mark.parametrize("log_m", [13, 14, 15, 16, 17])
def test_trees_of_the_throughput_kernel(zk, log_m):
    """Switch at 2^12: 2^13 .. 2^16 leaves are one leaf-mode launch of b2s_subtree_kernel with k = 1 .. 4 and the latency kernel in inner
    mode above it; 2^17 is the leaf launch (k = 4) and an inner-mode throughput launch (k = 1).  The smallest trees that reach both
    modes and every k."""
    m = 1 << log_m
    with _latency_log(zk.load(), 12):
        t = zk.Merkle(m, _leaves()[:m], hash="blake2s")
    _assert_nodes(t.nodes, _ref_tree(m), f"2^{log_m} leaves, switch at 2^12")


# ---- whole proofs ---------------------------------------------------------------------------------------------------------------
def _assert_proof(ctx, p, ref, what):
    assert (p.data, p.state) == (ref.data, ref.state), what
    assert p.check(strict=True) == 0 and p.check() == 0, what


def _assert_trees(ctx, ref, log_n, K, coset, D):
    """Every tree the proof committed, node for node (this is where the latency kernel's continuation runs: a context has a counter)."""
    steps_of = {0: 0, 1: 0}
    grp = blake2s_ref.groups(log_n - D, K)
    for j, (r0, steps) in enumerate(grp):
        if coset:
            steps_of[1 + r0] = steps
        if not (D and j + 1 == len(grp)):
            steps_of.setdefault(1 + r0 + steps, 0)
    for tid, want in ref.c.trees.items():
        _assert_nodes(ctx.merkle_nodes(tid, coset_steps=steps_of[tid]), want, f"tree {tid}")


CASES = [  # log_n, log_b, switch (0: default), K, coset, D, q, bits
    pytest.param(10, 3, 0, 1, False, 0, 1, 0, id="10-3-defaults"),
    pytest.param(11, 3, 12, 1, False, 0, 1, 0, id="11-3-switch12"),      # ComposeSrc (k = 2) and FoldSrc (k = 1) through b2s_subtree_kernel
    pytest.param(10, 3, 0, 2, True, 0, 1, 0, id="K2-coset"),
    pytest.param(10, 3, 0, 2, True, 3, 1, 0, id="K2-coset-D3"),
    pytest.param(10, 3, 0, 3, True, 0, 1, 0, id="K3-coset"),
    pytest.param(10, 3, 0, 3, True, 3, 1, 0, id="K3-coset-D3"),
    pytest.param(10, 3, 0, 1, False, 0, 3, 8, id="q3-grind8"),
    # 2^17-leaf trees: the largest the latency kernel takes alone (j = 9, j2 = 8), every continuation split below; seven queries
    pytest.param(14, 3, 0, 1, False, 0, 7, 0, id="14-3-q7"),
    # switch at 2^12: PlainSrc and ComposeSrc leaf launches of k = 4 with an inner launch of k = 1 above them, FoldSrc leaf launches of
    # k = 4, 3, 2, 1 on the 2^16 .. 2^13-leaf trees
    pytest.param(14, 3, 12, 1, False, 0, 1, 0, id="14-3-switch12"),
    # coset trees above the switch inside a proof: coset_leaf_hash_kernel<2, S>, then inner throughput launches
    pytest.param(13, 3, 12, 2, True, 0, 1, 0, id="13-3-switch12-K2-coset"),
    pytest.param(13, 3, 12, 3, True, 3, 1, 0, id="13-3-switch12-K3-coset-D3"),
]


@pytest.mark.parametrize("log_n,log_b,lat,K,coset,D,q,bits", CASES)
def test_zk_prove_is_the_reference_proof(zk, orc, log_n, log_b, lat, K, coset, D, q, bits):
    ref = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D, bits)
    trace = _trace(1 << log_n)
    with _latency_log(zk.load(), lat):
        with zk.Context(log_n, log_b, hash="blake2s", queries=q, grind_bits=bits, fold_log=K, coset_leaves=coset, stop_log=D) as ctx:
            p = ctx.prove(trace)
            _assert_proof(ctx, p, ref, "zk_prove")
            assert p.hash == "blake2s" and len(p.data) == stop_ref.proof_len(log_n, log_b, q, bits, K, coset, D)
            assert [int(v) for v in ctx.final_poly()] == ref.coef
            _assert_trees(ctx, ref, log_n, K, coset, D)
            again = ctx.prove(trace)                                  # a second proof on the same context
            _assert_proof(ctx, again, ref, "second proof")


A1_OTHER = 2718281


@pytest.mark.parametrize("log_n,log_b,lat", [pytest.param(10, 3, 0, id="10-3"), pytest.param(14, 3, 12, id="14-3-switch12")])
def test_early_launch_is_the_reference_proof(zk, orc, log_n, log_b, lat):
    """zk_ctx_set_early_launch with BLAKE2s: round r + 1's fold + commit launches (FoldSrc through merkle_wg_kernel<.., 2>, and at the
    lowered switch through b2s_subtree_kernel) are enqueued behind the gate word and read their challenge when they run.  The gated proof
    is the reference proof, so is a second proof of another trace on the same gated context, and so is the proof with the gate off again."""
    lib = zk.load()
    n = 1 << log_n
    ref, ref_other = blake2s_ref.proof(orc, log_n, log_b), blake2s_ref.proof(orc, log_n, log_b, a1=A1_OTHER)
    assert ref.data != ref_other.data
    with _latency_log(lib, lat):
        with zk.Context(log_n, log_b, hash="blake2s") as ctx:
            assert ctx.set_early_launch(True) is True and lib.zk_ctx_get_early_launch(ctx._h) == 1   # not silently off
            _assert_proof(ctx, ctx.prove(_trace(n)), ref, "gated proof")
            _assert_trees(ctx, ref, log_n, 1, False, 0)
            _assert_proof(ctx, ctx.prove(_trace(n, A1_OTHER)), ref_other, "gated proof of a second trace")
            _assert_trees(ctx, ref_other, log_n, 1, False, 0)
            assert lib.zk_ctx_get_early_launch(ctx._h) == 1
            assert ctx.set_early_launch(False) is False
            _assert_proof(ctx, ctx.prove(_trace(n)), ref, "the gate off again")
            _assert_trees(ctx, ref, log_n, 1, False, 0)


def test_channel_resident_and_many(zk, orc):
    """zk_prove_resident, zk_prove_channel behind a prefix and zk_prove_many on two contexts (K = 2, coset leaves, D = 3, two queries)."""
    log_n, log_b, K, coset, D, q = 10, 3, 2, True, 3, 2
    ref = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D)
    refp = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D, prefix=PREFIX)
    kw = dict(hash="blake2s", queries=q, fold_log=K, coset_leaves=coset, stop_log=D)
    with zk.Context(log_n, log_b, **kw) as a, zk.Context(log_n, log_b, **kw) as b:
        a.trace_upload(_trace(1 << log_n))
        b.trace_upload(_trace(1 << log_n))
        _assert_proof(a, a.prove(), ref, "zk_prove_resident")
        ch = zk.Channel()
        ch.commit(PREFIX)
        pc = b.prove_channel(ch)
        assert (pc.data, pc.state) == (refp.data, refp.state)
        for pm in zk.prove_many([a, b]):
            _assert_proof(a, pm, ref, "zk_prove_many")


def test_one_live_context_through_the_three_hashes(zk, orc):
    """sha256 -> blake2s -> field -> blake2s -> sha256 on one context: each proof is its reference."""
    log_n, log_b = 10, 3
    lib = zk.load()
    trace = _trace(1 << log_n)
    refs = {"sha256": stop_ref.stop_proof(orc, log_n, log_b, 1, 0, 1, False, 0), "field": stop_ref.stop_proof(orc, log_n, log_b, 1, 1, 1, False, 0),
            "blake2s": blake2s_ref.proof(orc, log_n, log_b)}
    assert refs["sha256"].data == orc.prove(log_n, log_b).proof       # the reference's own bytes
    with zk.Context(log_n, log_b) as ctx:
        for name in ("sha256", "blake2s", "field", "blake2s", "sha256"):
            assert lib.zk_ctx_set_hash(ctx._h, zk.host.HASHES[name]) == 0
            ctx.hash = name
            _assert_proof(ctx, ctx.prove(trace), refs[name], name)
        assert lib.zk_ctx_set_hash(ctx._h, 3) == ZK_ERR_INVALID
        _assert_proof(ctx, ctx.prove(trace), refs["sha256"], "after a refused kind")


def test_probe_runs_the_blake2s_chain(zk):
    r = zk.probe_hash_chain("blake2s", waves_per_simd=1, hashes=4, launches=2)
    assert r["ns_per_hash_per_simd"] > 0 and r["hashes"] == 4


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(lib, rc):
    assert rc == ZK_ERR_INVALID, rc
    assert b"BLAKE2s" in lib.zk_last_error(), lib.zk_last_error()


def test_batch_refuses_and_stays_usable(zk, orc):
    lib = zk.load()
    log_n, log_b = 6, 3
    want = orc.prove(log_n, log_b, 1, 3141592)
    with zk.BatchContext(log_n, log_b, 1) as b:
        _refused(lib, lib.zk_batch_set_hash(b._h, KIND))
        b.gen_fibsq([1, 1], [3141592, 3141592])
        for p in b.prove():
            assert (p.data, p.state) == (want.proof, want.state)


def test_shard_refuses_and_stays_usable(zk, orc):
    import os
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    lib = zk.load()
    log_n, log_b = 10, 3
    want = orc.prove(log_n, log_b)
    with zk.ShardContext(log_n, log_b, 0, 1, zk.shard_unique_id(), force_collectives=True, min_layer_log=1, min_chunk_log=4) as sp:
        _refused(lib, lib.zk_shard_set_hash(sp._h, KIND))
        sp.trace_upload(zk.trace_fibsq((1 << log_n) - 1))
        p = sp.prove()
        assert (p.data, p.state) == (want.proof, want.state)


def test_committer_and_chunk_builds_refuse_and_stay_usable(zk, orc):
    import torch
    lib = zk.load()
    dev = torch.device("cuda", 0)
    log_m = 6
    vals = _leaves()[:1 << log_m]
    d_vals = torch.from_numpy(vals.view(np.int32).copy()).to(dev)
    d_nodes = torch.zeros(((2 << log_m) - 1) * 8, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    root = C.create_string_buffer(32)
    k = C.c_void_p()
    assert lib.zk_committer_create(0, C.byref(k)) == 0
    try:
        _refused(lib, lib.zk_dev_merkle_commit(k, d_vals.data_ptr(), 0, log_m, d_nodes.data_ptr(), stream, KIND, root))
        _refused(lib, lib.zk_dev_merkle_commit(k, d_vals.data_ptr(), 2, log_m - 2, d_nodes.data_ptr(), stream, KIND, root))
        _refused(lib, lib.zk_dev_merkle_commit_finish(k, d_nodes.data_ptr(), log_m, 1, stream, KIND, root))
        _refused(lib, lib.zk_dev_merkle_build_chunk(d_vals.data_ptr(), 0, log_m - 1, d_nodes.data_ptr(), log_m, 0, stream, KIND))
        _refused(lib, lib.zk_dev_merkle_finish(d_nodes.data_ptr(), log_m, 1, stream, KIND))
        _refused(lib, lib.zk_dev_merkle_build_interleaved(d_vals.data_ptr(), 2, log_m - 2, d_nodes.data_ptr(), stream, KIND))
        torch.cuda.current_stream(dev).synchronize()
        assert not d_nodes.any().item()                               # nothing was launched
        # the committer still commits: SHA-256 against the oracle, and the plain build takes the new hash
        assert lib.zk_dev_merkle_commit(k, d_vals.data_ptr(), 0, log_m, d_nodes.data_ptr(), stream, 0, root) == 0
        assert root.raw == bytes(orc.merkle_build(vals)[0])
        assert lib.zk_dev_merkle_build_ex(d_vals.data_ptr(), log_m, d_nodes.data_ptr(), stream, KIND) == 0
        torch.cuda.current_stream(dev).synchronize()
        got = d_nodes.cpu().numpy().view(np.uint32).reshape(-1, 8).astype(">u4").view(np.uint8).reshape(-1, 32)
        _assert_nodes(got, _ref_tree(1 << log_m), "zk_dev_merkle_build_ex")
    finally:
        lib.zk_committer_destroy(k)
