"""Coset leaves on the GPU (zk_ctx_set_coset_leaves, zk_merkle_commit_coset): coset_leaf_hash_kernel and the build
above it against the plain-Python tree of tests/coset_ref.py node for node, and every one-call prover against the proofs
coset_ref builds without the library -- bytes and final state."""
import ctypes as C
import functools

import numpy as np
import pytest

import coset_ref
import fold_ref
from transforms_ref import P, rand_field

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
HOST_LEVELS = ((0, 0), (8, 9), (10, 9))                      # device only; the default; a hand-over two levels deeper


def _trace(n, a1=3141592):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


def _layer(log_len):
    v = rand_field(np.random.default_rng(1000 + log_len), 1 << log_len)
    v[0], v[-1] = 0, P - 1                                    # zk_layer_write admits canonical residues only: no raw words >= P
    return v


@functools.lru_cache(maxsize=None)
def _ref_tree(log_len, steps, hash_kind):
    import oracle as orc
    orc.set_hash(hash_kind)
    try:
        nodes = coset_ref.tree(orc, _layer(log_len), steps, hash_kind)
    finally:
        orc.set_hash(0)
    nodes.setflags(write=False)
    return nodes


def _layer_of(ctx, log_len):
    """The FRI layer id of `ctx` that holds 2^log_len values."""
    L = ctx.log_n + ctx.log_blowup
    assert L - ctx.log_n <= log_len <= L
    return 1 + (L - log_len)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("steps", [0, 1, 2, 3])
def test_coset_tree_matches_python_tree_node_for_node(zk, steps, hash_kind):
    """Layers of 2^(1 + steps) .. 2^13 values: the one-leaf-pair tree, the workgroup-local path, and both sides of the 2^8 / 2^9 /
    2^10 hand-over depths under three host-level settings; then paths of the first, the last and 32 random leaves."""
    rng = np.random.default_rng(steps)
    with zk.Context(10, 3, hash=HASH_NAMES[hash_kind]) as big, zk.Context(2, 1, hash=HASH_NAMES[hash_kind]) as small:
        for log_len in range(1 + steps, 14):
            ctx = big if log_len >= 3 else small
            lid = _layer_of(ctx, log_len)
            want = _ref_tree(log_len, steps, hash_kind)
            ctx.layer_write(lid, _layer(log_len))
            for hl in HOST_LEVELS:
                ctx.set_host_levels(*hl)
                root = ctx.merkle_commit(lid, coset_steps=steps)
                got = ctx.merkle_nodes(lid, coset_steps=steps)
                assert got.shape == want.shape and root == bytes(want[0]), (log_len, hl)
                assert np.array_equal(got, want), (log_len, hl, int(np.argmax((got != want).any(axis=1))))
            m = 1 << (log_len - steps)
            for leaf in sorted({0, m - 1} | set(int(x) for x in rng.integers(0, m, 32))):
                assert ctx.merkle_path(lid, leaf) == coset_ref.path(want, leaf), (log_len, leaf)
            with pytest.raises(zk.ZkError):
                ctx.merkle_path(lid, m)                      # a coset tree is addressed by its own leaves
            # the same layer committed with one-value leaves again: the tree read-outs follow what was built last
            if steps:
                ctx.merkle_commit(lid)
                assert ctx.merkle_nodes(lid).shape[0] == 2 * (1 << log_len) - 1
        with pytest.raises(zk.ZkError):
            big.merkle_commit(11, coset_steps=3)             # 2^3 values, steps 3: a single leaf is no tree
        with pytest.raises(zk.ZkError):
            big.merkle_commit(1, coset_steps=4)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("steps", [3, 1])
def test_large_coset_tree_reaches_the_throughput_launches(zk, steps, hash_kind):
    """A layer of 2^21 values: the root, and 4 096 sampled leaves -- their digests in the heap and their paths -- checked with
    zk_compute_root_from_coset."""
    log_len, lib = 21, zk.load()
    m, s = 1 << (log_len - steps), 1 << steps
    layer = rand_field(np.random.default_rng(21 + steps), 1 << log_len)
    with zk.Context(18, 3, hash=HASH_NAMES[hash_kind]) as ctx:
        ctx.layer_write(1, layer)
        root = ctx.merkle_commit(1, coset_steps=steps)
        nodes = ctx.merkle_nodes(1, coset_steps=steps)
    assert nodes.shape == (2 * m - 1, 32) and bytes(nodes[0]) == root
    out = C.create_string_buffer(32)
    rng = np.random.default_rng(steps)
    for leaf in sorted({0, m - 1} | set(int(x) for x in rng.integers(0, m, 4094))):
        slots = np.ascontiguousarray(layer[leaf::m][:s])
        assert len(slots) == s
        pth = b"".join(coset_ref.path(nodes, leaf))
        assert lib.zk_compute_root_from_coset(slots.ctypes.data_as(C.c_void_p), s, leaf, pth, 0, out, hash_kind) == 0
        assert out.raw == bytes(nodes[m - 1 + leaf]), leaf
        assert lib.zk_compute_root_from_coset(slots.ctypes.data_as(C.c_void_p), s, leaf, pth, len(pth) // 32, out, hash_kind) == 0
        assert out.raw == root, leaf


PREFIX = b"coset leaves: a transcript prefix"


def _prove_prefixed(zk, ctx):
    ch = zk.Channel()
    ch.commit(PREFIX)
    return ctx.prove_channel(ch)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("log_n,log_b", [(4, 1), (5, 2), (6, 3), (10, 3), (12, 3)])
def test_proofs_are_the_reference_proofs(zk, orc, log_n, log_b, K, hash_kind):
    """zk_prove, zk_prove_channel on a non-empty prefix and zk_prove_many on two contexts, q in {1, 4}, grind 0 and 12, device-only
    trees and the default hand-over: byte for byte coset_ref's proof and the same final state."""
    trace = _trace(1 << log_n)
    kw = dict(hash=HASH_NAMES[hash_kind], fold_log=K, coset_leaves=True)
    lib = zk.load()
    with zk.Context(log_n, log_b, **kw) as a, zk.Context(log_n, log_b, **kw) as b:
        assert lib.zk_ctx_get_coset_leaves(a._h) == 1 and lib.zk_ctx_get_early_launch(a._h) == 0
        b.trace_upload(trace)
        default_levels = a.host_levels
        for hl in ((0, 0), default_levels):
            a.set_host_levels(*hl)
            b.set_host_levels(*hl)
            for q in (1, 4):
                for g in (0, 12):
                    for c in (a, b):
                        assert lib.zk_ctx_set_queries(c._h, q) == 0 and lib.zk_ctx_set_grinding(c._h, g) == 0
                        c.queries, c.grind_bits = q, g
                    ref = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, g)
                    p = a.prove(trace)
                    assert (p.data, p.state) == (ref.data, ref.state), (hl, q, g)
                    assert len(p.data) == p.expected_len() == coset_ref.proof_len(log_n, log_b, q, g, K)
                    assert p.check(strict=True) == 0 and p.check() == 0
                    for pm in zk.prove_many([a, b]):
                        assert (pm.data, pm.state) == (ref.data, ref.state), ("many", hl, q, g)
                    refp = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, g, prefix=PREFIX)
                    pc = _prove_prefixed(zk, b)
                    assert (pc.data, pc.state) == (refp.data, refp.state), ("channel", hl, q, g)


def test_switching_on_one_live_context(zk, orc):
    """Coset leaves on / off and K 1 -> 3 -> 2 -> 1 between proofs of one context: every proof is its reference, and with the
    option off the bytes are the one-value-leaf format's (fold_ref)."""
    log_n, log_b = 10, 3
    trace = _trace(1 << log_n)
    with zk.Context(log_n, log_b) as ctx:
        for rep in range(2):
            for K in (1, 3, 2, 1):
                ctx.set_fold(K)
                for on in (True, False, True):
                    ctx.set_coset_leaves(on)
                    p = ctx.prove(trace)
                    ref = coset_ref.coset_proof(orc, log_n, log_b, 1, 0, K) if on else fold_ref.fold_proof(orc, log_n, log_b, 1, 0, K)
                    assert (p.data, p.state) == (ref.data, ref.state), (rep, K, on)
                    p.verify(strict=True)
        ctx.set_coset_leaves(False)
        ctx.set_fold(1)
        assert ctx.prove(trace).data == orc.prove(log_n, log_b).proof


@pytest.mark.parametrize("K", [3, 1])
def test_one_proof_at_domain_2e22(zk, K):
    log_n, log_b, q = 19, 3, 8
    with zk.Context(log_n, log_b, queries=q, fold_log=K, coset_leaves=True) as ctx:
        p = ctx.prove(_trace(1 << log_n))
    assert len(p.data) == zk.load().zk_proof_data_len_coset(log_n, log_b, q, 0, K) == coset_ref.proof_len(log_n, log_b, q, 0, K)
    assert p.check(strict=True) == 0
    p.verify(strict=True)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
def test_self_checks_pass_with_coset_leaves(zk, orc, hash_kind):
    log_n, log_b = 10, 3
    for K in (1, 2, 3):
        with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], fold_log=K, coset_leaves=True) as ctx:
            ctx.set_checks(True)
            p = ctx.prove(_trace(1 << log_n))
        ref = coset_ref.coset_proof(orc, log_n, log_b, 1, hash_kind, K)
        assert (p.data, p.state) == (ref.data, ref.state)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_generate_proof_stage_by_stage(zk, orc, K):
    """generate_proof on a context with coset leaves on: the stage calls (zk_merkle_commit_coset, zk_fri_fold_multi, zk_merkle_path on
    coset trees) assemble the same proof."""
    log_n, log_b = 6, 3
    with zk.Context(log_n, log_b, fold_log=K, coset_leaves=True) as ctx:
        p = zk.generate_proof(zk.Channel(), log_n, log_b, ctx=ctx)
    ref = coset_ref.coset_proof(orc, log_n, log_b, 1, 0, K)
    assert (p.data, p.state) == (ref.data, ref.state)
    p.verify(strict=True)
