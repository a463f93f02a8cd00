"""One live prover context walked through every pair of its settings (tests/settings_walk.py; DESIGN.md 7d "Reconfiguring a live
context"), Merkle caps, BLAKE2s and challenges in E among them: after every setter call the next proof is the reference proof of the new
configuration byte for byte, the final polynomial, the challenges and the read-outs of layers, caps and tree nodes are this proof's or
answer ZK_ERR_STATE, a failed proof in between leaves nothing behind, and hash and extension are set in the one order the library allows."""
import ctypes as C

import numpy as np
import pytest

import fold_ref
import settings_walk as sw
from transforms_ref import P

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field", 2: "blake2s"}
ZK_ERR_INVALID, ZK_ERR_STATE, ZK_ERR_CHECK = -1, -4, -7
FRESH = sw.Step(hash=0, q=1, bits=0, K=1, coset=False, D=0, host="default", early=False, checks=False, entry=None, a1=None, cap=0, ext=0)


def _trace(zk, log_n, a1):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


def _wrong_order(prev, step):
    """The setter that zk_ctx must refuse when it comes first: leaving BLAKE2s for ext the hash has to change first, entering BLAKE2s from
    ext the extension has to go first (None: any order is legal)."""
    if prev.hash == 2 and step.ext == 1:
        return "ext"
    if prev.ext == 1 and step.hash == 2:
        return "hash"
    return None


def _refused_setter(lib, ctx, prev, step):
    """At a hash_ext_order transition: the wrong setter first is ZK_ERR_INVALID, names both settings, and changes neither."""
    first = _wrong_order(prev, step)
    rc = lib.zk_ctx_set_ext(ctx._h, 1) if first == "ext" else lib.zk_ctx_set_hash(ctx._h, 2)
    assert rc == ZK_ERR_INVALID, (prev, step, rc)
    msg = lib.zk_last_error()
    assert b"ext_log" in msg and b"BLAKE2s" in msg, msg
    assert lib.zk_ctx_get_ext(ctx._h) == prev.ext


def _configure(lib, ctxs, step, prev, default_levels):
    """The setters of the factors that differ from `prev`.  Hash and extension in the one legal order: towards BLAKE2s the extension goes
    first, in every other case the hash does."""
    def changed(f):
        return getattr(prev, f) != getattr(step, f)

    for c in ctxs:
        def set_hash():
            if changed("hash"):
                assert lib.zk_ctx_set_hash(c._h, step.hash) == 0
                c.hash = HASH_NAMES[step.hash]

        def set_ext():
            if changed("ext"):
                c.set_ext(step.ext)

        for setter in ((set_ext, set_hash) if step.hash == 2 else (set_hash, set_ext)):
            setter()
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
        if changed("cap"):
            c.set_merkle_cap(step.cap)
        if changed("host"):
            c.set_host_levels(*sw.host_levels(step.host, default_levels))
        if changed("early"):
            c.set_early_launch(step.early)
        if changed("checks"):
            c.set_checks(step.checks)
        assert lib.zk_ctx_get_ext(c._h) == step.ext and lib.zk_ctx_get_merkle_cap(c._h) == step.cap, step


def _check_readouts(lib, ctx, ref, step, log_n, log_b):
    """Every layer, cap and tree node the context hands out is this proof's; what this proof did not make is ZK_ERR_STATE."""
    L, Rp = log_n + log_b, log_n - step.D
    info = ctx.last_transcript()
    for lid in range(log_n + 2):
        out = np.zeros(ctx.layer_size(lid), dtype=np.uint32)
        rc = lib.zk_layer_read(ctx._h, lid, 0, len(out), out.ctypes.data_as(C.c_void_p))
        if lid in ref.layers and not (step.ext and lid):      # committed layers and the stopped one; with ext only f is a base-field layer
            assert rc == 0 and np.array_equal(out, ref.layers[lid]), ("layer", lid)
        else:
            assert rc == ZK_ERR_STATE, ("layer", lid, rc)     # a success here could only be an earlier proof's values
        buf, caps = C.create_string_buffer(32), np.zeros(32 << 8, dtype=np.uint8)
        rc_node = lib.zk_merkle_node(ctx._h, lid, 0, buf)
        rc_cap = lib.zk_ctx_merkle_cap(ctx._h, lid, caps.ctypes.data_as(C.c_void_p), caps.size)
        if lid not in ref.trees:
            assert (rc_node, rc_cap) == (ZK_ERR_STATE, ZK_ERR_STATE), ("tree", lid, rc_node, rc_cap)
            continue
        ce, heap = ref.ce[lid], ref.trees[lid]
        assert ce == min(step.cap, ref.lg[lid] - 1) and lib.zk_ctx_merkle_cap_log(ctx._h, lid) == ce, ("cap depth", lid)
        assert rc_cap == 0 and caps[:32 << ce].tobytes() == ref.caps[lid], ("cap", lid)
        if ce:
            assert rc_node == ZK_ERR_STATE and bytes(info.roots[lid]) == bytes(32), ("root above the cap", lid, rc_node)
        else:
            assert rc_node == 0 and buf.raw == ref.caps[lid] == bytes(heap[0]) == bytes(info.roots[lid]), ("root", lid)
        # the nodes from the cap's depth down: the whole heap at (6, 3); down to depth 11 at (10, 3) -- every level the host may
        # build (at most 10 below the root) and one device level under it
        first = (1 << ce) - 1
        end = len(heap) if log_n <= 6 else min(len(heap), (1 << 12) - 1)
        steps = L - max(lid - 1, 0) - ref.lg[lid]             # slots per leaf, as a logarithm: what the tree was built with
        got = ctx.merkle_nodes(lid, first, end - first, coset_steps=steps)
        assert np.array_equal(got, heap[first:end]), ("nodes", lid, first, end)
    assert 1 + Rp in ref.layers and {0, 1} <= set(ref.trees)
    if step.D:                                                # past the stop nothing exists (tests/test_gpu_fri_stop.py pins the same)
        assert set(range(2 + Rp, log_n + 2)).isdisjoint(ref.layers) and set(range(1 + Rp, log_n + 2)).isdisjoint(ref.trees)


def _check_transcript(ctx, ref, step, log_n):
    """The final polynomial and the challenges the context reports are this proof's; no component-1 raw outlives an ext proof."""
    info = ctx.last_transcript()
    assert list(ctx.final_poly()) == ref.coef and len(ref.coef) == 1 << (step.D + step.ext)
    assert info.free_term == ref.coef[0]
    assert list(info.alpha_raw) == ref.alphas
    grp = fold_ref.groups(log_n - step.D, step.K)
    assert sorted(ref.betas) == [r0 for r0, _ in grp] and [info.beta_raw[r0] for r0, _ in grp] == [ref.betas[r0] for r0, _ in grp]
    assert ctx.ext_challenges() == ref.ext_challenges and len(ref.ext_challenges) == (3 + len(grp) if step.ext else 0)


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

            prev, refused = FRESH, []
            for i, step in enumerate(steps):
                what = (i, step)
                print("step", i, step)                        # shown with a failure: (predecessor, step) is the reproduction
                if _wrong_order(prev, step):                  # the refused setter changes nothing: the next proof is the previous step's again
                    _refused_setter(lib, ctx, prev, step)
                    same = sw.expected(orc, (log_n, log_b), prev._replace(entry="prove_trace"))
                    again = ctx.prove(traces[prev.a1])
                    resident[ctx] = prev.a1
                    assert (again.data, again.state) == (same.data, same.state), what
                    assert ctx.ext_challenges() == same.ext_challenges, what
                    refused.append(i)
                _configure(lib, (ctx, other), step, prev, default_levels)
                prev = step
                assert lib.zk_ctx_get_early_launch(ctx._h) == int(step.early and can_early and sw.fmt(step) == (1, False, 0) and not step.ext), what
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
                        p = zk.Proof(p.state, p.data[len(pre):], log_n, log_b, p.public_last, ctx.hash, step.q, step.bits, step.K, step.coset, step.D,
                                     cap_log=step.cap, ext_log=step.ext)
                        assert p.check() == 0, what
                    else:
                        assert (p.cap_log, p.ext_log) == (step.cap, step.ext) and p.check(strict=True) == 0, what
                for c in (ctx, other) if step.entry == "prove_many" else (ctx,):
                    _check_transcript(c, ref, step, log_n)
                _check_readouts(lib, ctx, ref, step, log_n, log_b)
            ways = sw.hash_ext_order(steps)
            assert set(ways["to_ext"] + ways["to_blake2s"]) <= set(refused) and ways["to_ext"] and ways["to_blake2s"], (ways, refused)
    finally:
        sw.forget_commits()


def test_decommitment_buffers_without_growing_them_first(zk, orc):
    """A fresh (10, 3) context, whose decommitment buffers were sized for K = 1: 64 queries with coset leaves at the largest stop, then
    the plain full format, then K = 3 with coset leaves.  "gather capacity exceeded" would contradict the comments in
    zk_ctx_set_coset_leaves and zk_ctx_set_fri_stop.  A second fresh context takes the buffers through zk_ctx_set_ext, which sizes them
    both ways: ext on at K = 1, K = 3 with one-value leaves (the largest fetch there is: two words per value, 2^3 values and paths per
    group), ext off at K = 3, back to K = 1, ext on again with coset leaves at the largest stop."""
    log_n, log_b, q = 10, 3, 64
    lib = zk.load()
    trace = _trace(zk, log_n, 3141592)
    dmax = sw.largest_stop(log_n, log_b)

    def prove_and_compare(ctx, K, coset, D, ext):
        if K != ctx.fold_log:
            ctx.set_fold(K)
        ctx.set_coset_leaves(coset)
        ctx.set_fri_stop(D)
        ref = sw.expected(orc, (log_n, log_b), sw.Step(0, q, 0, K, coset, D, "default", False, False, "prove_trace", 3141592, 0, ext))
        p = ctx.prove(trace)                                  # a ZkError "gather capacity exceeded" ends the test here
        assert (p.data, p.state) == (ref.data, ref.state), (K, coset, D, ext)
        assert p.check(strict=True) == 0
        assert list(ctx.final_poly()) == ref.coef and ctx.ext_challenges() == ref.ext_challenges, (K, coset, D, ext)

    try:
        with zk.Context(log_n, log_b) as ctx:
            assert lib.zk_ctx_set_queries(ctx._h, q) == 0
            ctx.queries = q
            for K, coset, D in ((1, True, dmax), (1, False, 0), (3, True, 0)):
                prove_and_compare(ctx, K, coset, D, 0)
        with zk.Context(log_n, log_b) as ctx:
            assert lib.zk_ctx_set_queries(ctx._h, q) == 0
            ctx.queries = q
            for ext, K, coset, D in ((1, 1, False, 0), (1, 3, False, 0), (0, 3, False, 0), (0, 1, False, 0), (1, 1, True, dmax)):
                ctx.set_ext(ext)                              # before set_fold: the order of the sequence, setter by setter
                assert lib.zk_ctx_get_ext(ctx._h) == ext
                prove_and_compare(ctx, K, coset, D, ext)
    finally:
        sw.forget_commits()
