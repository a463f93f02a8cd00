"""One live prover context walked through every pair of its settings (tests/settings_walk.py; DESIGN.md 7d "Reconfiguring a live
context"): after every setter call the next proof is the reference proof of the new configuration byte for byte, the final polynomial
and the read-outs of layers and trees are this proof's or answer ZK_ERR_STATE, and a failed proof in between leaves nothing behind."""
import ctypes as C

import numpy as np
import pytest

import settings_walk as sw
from transforms_ref import P

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ZK_ERR_STATE, ZK_ERR_CHECK = -4, -7


def _trace(zk, log_n, a1):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


def _configure(lib, ctxs, step, prev, default_levels):
    """The setters of the factors that differ from `prev` (None: a fresh context, whose settings are the library's defaults)."""
    if prev is None:
        prev = sw.Step(hash=0, q=1, bits=0, K=1, coset=False, D=0, host="default", early=False, checks=False, entry=None, a1=None)

    def changed(f):
        return getattr(prev, f) != getattr(step, f)

    for c in ctxs:
        if changed("hash"):
            assert lib.zk_ctx_set_hash(c._h, step.hash) == 0
            c.hash = HASH_NAMES[step.hash]
        if changed("q"):
            assert lib.zk_ctx_set_queries(c._h, step.q) == 0
            c.queries = step.q
        if changed("bits"):
            assert lib.zk_ctx_set_grinding(c._h, step.bits) == 0
            c.grind_bits = step.bits
        if changed("K"):
            c.set_fold(step.K)
        if changed("coset"):
            c.set_coset_leaves(step.coset)
        if changed("D"):
            c.set_fri_stop(step.D)
        if changed("host"):
            c.set_host_levels(*sw.host_levels(step.host, default_levels))
        if changed("early"):
            c.set_early_launch(step.early)
        if changed("checks"):
            c.set_checks(step.checks)


def _check_readouts(lib, ctx, ref, step, log_n):
    """Step 5: every layer and every tree root the context hands out is this proof's; what this proof did not make is ZK_ERR_STATE."""
    Rp = log_n - step.D
    for lid in range(log_n + 2):
        out = np.zeros(ctx.layer_size(lid), dtype=np.uint32)
        rc = lib.zk_layer_read(ctx._h, lid, 0, len(out), out.ctypes.data_as(C.c_void_p))
        if lid in ref.c.layers:                               # committed layers and the stopped one
            assert rc == 0 and np.array_equal(out, ref.c.layers[lid]), ("layer", lid)
        else:
            assert rc == ZK_ERR_STATE, ("layer", lid, rc)     # a success here could only be an earlier proof's values
        buf = C.create_string_buffer(32)
        rc = lib.zk_merkle_node(ctx._h, lid, 0, buf)
        if lid in ref.c.roots:
            assert rc == 0 and buf.raw == ref.c.roots[lid], ("root", lid)
        else:
            assert rc == ZK_ERR_STATE, ("root", lid, rc)
    assert 1 + Rp in ref.c.layers and {0, 1} <= set(ref.c.roots)
    if step.D:                                                # past the stop nothing exists (tests/test_gpu_fri_stop.py pins the same)
        assert set(range(2 + Rp, log_n + 2)).isdisjoint(ref.c.layers) and set(range(1 + Rp, log_n + 2)).isdisjoint(ref.c.roots)


@pytest.mark.parametrize("log_n,log_b", [(6, 3), (10, 3)])
def test_walk_on_one_live_context(zk, orc, log_n, log_b):
    lib = zk.load()
    steps = sw.walk(log_n, log_b)
    faults = sw.fault_steps(steps)
    traces = {a1: _trace(zk, log_n, a1) for a1 in sw.values(log_n, log_b)["a1"]}
    try:
        with zk.Context(log_n, log_b) as ctx, zk.Context(log_n, log_b) as other:
            default_levels = ctx.host_levels
            can_early = ctx.set_early_launch(True)            # on a fresh context: whether the device supports it
            ctx.set_early_launch(False)
            resident = {ctx: None, other: None}               # the a1 of the trace each context holds

            def upload(c, a1):
                if resident[c] != a1:
                    c.trace_upload(traces[a1])
                    resident[c] = a1

            prev = None
            for i, step in enumerate(steps):
                what = (i, step)
                _configure(lib, (ctx, other), step, prev, default_levels)
                prev = step
                assert lib.zk_ctx_get_early_launch(ctx._h) == int(step.early and can_early and sw.fmt(step) == (1, False, 0)), what
                ref = sw.expected(orc, (log_n, log_b), step)
                if i in faults:                               # a proof that fails, in this configuration, before the good one
                    bad = traces[step.a1].copy()
                    bad[(1 << log_n) // 2] = (int(bad[(1 << log_n) // 2]) + 1) % P
                    with pytest.raises(zk.ZkError) as e:
                        ctx.prove(bad)
                    assert e.value.code == ZK_ERR_CHECK and sw.fault_message(step) in str(e.value), (what, str(e.value))
                    resident[ctx] = None
                pre = sw.prefix_of(step)
                if step.entry == "prove_trace":
                    proofs = [ctx.prove(traces[step.a1])]
                    resident[ctx] = step.a1
                elif step.entry == "prove_resident":
                    upload(ctx, step.a1)
                    proofs = [ctx.prove()]
                elif step.entry == "prove_channel":
                    upload(ctx, step.a1)
                    ch = zk.Channel()
                    ch.commit(pre)
                    proofs = [ctx.prove_channel(ch)]
                else:
                    upload(ctx, step.a1)
                    upload(other, step.a1)
                    proofs = zk.prove_many([ctx, other])
                    assert len(proofs) == 2
                for p in proofs:
                    assert (p.data, p.state) == (ref.data, ref.state), what
                    assert len(p.data) == ctx._proof_cap() + len(pre), what
                    if pre:                                   # behind a prefix: the proof is what follows it, and only the lax verifier applies
                        p = zk.Proof(p.state, p.data[len(pre):], log_n, log_b, p.public_last, ctx.hash, step.q, step.bits, step.K, step.coset, step.D)
                        assert p.check() == 0, what
                    else:
                        assert p.check(strict=True) == 0, what
                assert list(ctx.final_poly()) == ref.coef and len(ref.coef) == 1 << step.D, what
                assert ctx.last_transcript().free_term == ref.coef[0], what
                _check_readouts(lib, ctx, ref, step, log_n)
    finally:
        sw.forget_commits()


def test_decommitment_buffers_without_growing_them_first(zk, orc):
    """A fresh (10, 3) context, whose decommitment buffers were sized for K = 1: 64 queries with coset leaves at the largest stop, then
    the plain full format, then K = 3 with coset leaves.  "gather capacity exceeded" would contradict the comments in
    zk_ctx_set_coset_leaves and zk_ctx_set_fri_stop."""
    log_n, log_b, q = 10, 3, 64
    lib = zk.load()
    trace = _trace(zk, log_n, 3141592)
    dmax = sw.largest_stop(log_n, log_b)
    try:
        with zk.Context(log_n, log_b) as ctx:
            assert lib.zk_ctx_set_queries(ctx._h, q) == 0
            ctx.queries = q
            for K, coset, D in ((1, True, dmax), (1, False, 0), (3, True, 0)):
                if K != ctx.fold_log:
                    ctx.set_fold(K)
                ctx.set_coset_leaves(coset)
                ctx.set_fri_stop(D)
                ref = sw.expected(orc, (log_n, log_b), sw.Step(0, q, 0, K, coset, D, "default", False, False, "prove_trace", 3141592))
                p = ctx.prove(trace)
                assert (p.data, p.state) == (ref.data, ref.state), (K, coset, D)
                assert p.check(strict=True) == 0
    finally:
        sw.forget_commits()
