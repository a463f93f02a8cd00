"""Early stop of FRI on the GPU (zk_ctx_set_fri_stop, zk_fri_final_poly; DESIGN.md 7d "Early stop"): fri_final_poly_kernel against a
host evaluation of what it returns, and the one-call provers against the proofs tests/stop_ref.py builds without the library --
bytes, final state and final polynomial."""
import ctypes as C

import numpy as np
import pytest

import stop_ref
from transforms_ref import P, rand_field

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ZK_ERR_INVALID, ZK_ERR_STATE, ZK_ERR_CHECK = -1, -4, -7


def _trace(n, a1=3141592):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


# (log_n, log_b, FRI layer id): layers of M = 4 (fewer values than lanes), 64, 128 (the wave boundary: 64 butterflies) and 4096 values.
# 4096 is the kernel's limit and is reached exactly, with log_n = 10, log_b = 4 (layer 3 of a 2^14 domain).
KERNEL_LAYERS = [(4, 1, 4), (10, 4, 9), (10, 4, 8), (10, 4, 3)]


@pytest.mark.parametrize("log_n,log_b,layer", KERNEL_LAYERS, ids=["M4", "M64", "M128", "M4096"])
def test_kernel_interpolates_random_layers(zk, log_n, log_b, layer):
    """Random residues in a FRI layer: the M returned coefficients, evaluated at the layer's M points on the host, reproduce all M
    values, and high_nonzero is the host's count for bound 1, M / 2 and M."""
    xs = stop_ref.points(log_n, log_b, layer - 1)
    M = len(xs)
    assert M == (4, 64, 128, 4096)[KERNEL_LAYERS.index((log_n, log_b, layer))]
    vals = rand_field(np.random.default_rng(M), M)
    vals[0], vals[-1] = 0, P - 1
    with zk.Context(log_n, log_b) as ctx:
        ctx.layer_write(layer, vals)
        for bound in (1, M // 2, M):
            coef, high = ctx.fri_final_poly(layer, bound)
            assert coef.shape == (M,) and (coef < P).all()
            assert np.array_equal(stop_ref.evaluate(coef, xs), vals.astype(np.uint64)), bound
            assert high == int(np.count_nonzero(coef[bound:])), bound
        assert np.array_equal(ctx.layer_read(layer), vals)        # the layer itself is left alone


@pytest.mark.parametrize("log_n,log_b,layer", KERNEL_LAYERS, ids=["M4", "M64", "M128", "M4096"])
def test_kernel_returns_a_known_polynomial(zk, log_n, log_b, layer):
    """The layer is the evaluation of a known random polynomial of degree < 2^D = M / 2^log_b: exactly those coefficients, 0 above."""
    xs = stop_ref.points(log_n, log_b, layer - 1)
    M = len(xs)
    deg = M >> log_b
    want = rand_field(np.random.default_rng(7 * M), deg)
    want[-1] = P - 1                                              # the top coefficient is not zero
    with zk.Context(log_n, log_b) as ctx:
        ctx.layer_write(layer, stop_ref.evaluate(want, xs).astype(np.uint32))
        coef, high = ctx.fri_final_poly(layer, deg)
        assert np.array_equal(coef[:deg], want) and not coef[deg:].any() and high == 0
        assert ctx.fri_final_poly(layer, deg - 1)[1] == 1 and ctx.fri_final_poly(layer, 0)[1] == int(np.count_nonzero(want))
        # out of range: layer 0, a layer past the last, a layer of more than 4096 values
        lib, out, hi = zk.load(), np.zeros(1 << 13, dtype=np.uint32), C.c_uint32()
        assert lib.zk_fri_final_poly(ctx._h, 0, 0, out.ctypes.data_as(C.c_void_p), C.byref(hi)) == ZK_ERR_INVALID
        assert lib.zk_fri_final_poly(ctx._h, log_n + 2, 0, out.ctypes.data_as(C.c_void_p), C.byref(hi)) == ZK_ERR_INVALID
        if log_n + log_b > 12:
            assert lib.zk_fri_final_poly(ctx._h, 1 + (log_n + log_b - 13), 0, out.ctypes.data_as(C.c_void_p), C.byref(hi)) == ZK_ERR_INVALID


# Every layer size the kernel accepts, M = 2 .. 4096: the workgroup is 64 lanes up to M = 128, then M / 2 lanes up to the cap of 1024 at
# M = 2048 (reached exactly), then two butterflies per lane at M = 4096; every loop strides by the workgroup size.  M = 4 .. 32 occur in
# both contexts, under two domain sizes and so two shifts s and two twiddle strides.
ALL_SIZES = [(4, 1, layer) for layer in range(1, 6)] + [(10, 2, layer) for layer in range(1, 12)]


@pytest.fixture(scope="module")
def size_contexts(zk):
    with zk.Context(4, 1) as small, zk.Context(10, 2) as big:
        yield {(4, 1): small, (10, 2): big}


def test_all_sizes_reach_every_layer_log():
    logs = [ln + lb - (layer - 1) for ln, lb, layer in ALL_SIZES]
    assert sorted(set(logs)) == list(range(1, 13)) and sorted(lg for lg in logs if logs.count(lg) == 2) == [2, 2, 3, 3, 4, 4, 5, 5]


@pytest.mark.parametrize("log_n,log_b,layer", ALL_SIZES, ids=[f"{ln}-{lb}-M{1 << (ln + lb - layer + 1)}" for ln, lb, layer in ALL_SIZES])
def test_kernel_at_every_size(size_contexts, log_n, log_b, layer):
    """Random residues with 0 and P - 1 among them: the M coefficients evaluate back to the layer at its M points, high_nonzero is the
    host's count for every bound in {0, 1, M / 2, M - 1, M}, the layer is left alone; then the evaluation of a known polynomial of degree
    < M / 2^log_b comes back coefficient for coefficient.  Integers in the field: equality, no tolerance."""
    ctx = size_contexts[(log_n, log_b)]
    xs = stop_ref.points(log_n, log_b, layer - 1)
    M = len(xs)
    assert M == 1 << (log_n + log_b - (layer - 1)) == ctx.layer_size(layer)
    vals = rand_field(np.random.default_rng(1000 * log_n + M), M)
    vals[0], vals[-1] = 0, P - 1
    ctx.layer_write(layer, vals)
    for bound in sorted({0, 1, M // 2, M - 1, M}):
        coef, high = ctx.fri_final_poly(layer, bound)
        assert coef.shape == (M,) and (coef < P).all()
        assert np.array_equal(stop_ref.evaluate(coef, xs), vals.astype(np.uint64)), bound
        assert high == int(np.count_nonzero(coef[bound:])), bound
    assert np.array_equal(ctx.layer_read(layer), vals)
    deg = M >> log_b
    want = rand_field(np.random.default_rng(7 * M + log_n), deg)
    want[-1] = P - 1
    known = stop_ref.evaluate(want, xs).astype(np.uint32)
    ctx.layer_write(layer, known)
    coef, high = ctx.fri_final_poly(layer, deg)
    assert np.array_equal(coef[:deg], want) and not coef[deg:].any() and high == 0
    assert ctx.fri_final_poly(layer, 0)[1] == int(np.count_nonzero(want)) and ctx.fri_final_poly(layer, deg - 1)[1] == 1
    assert np.array_equal(ctx.layer_read(layer), known)


SHAPES = ([(ln, lb, D) for ln, lb in ((4, 1), (5, 2), (6, 3)) for D in sorted({1, 2, ln - 1})]
          + [(10, 3, 4), (10, 3, 8), (9, 3, 8)])                  # (9, 3, 8): R' = 1, one group of one step for every K


@pytest.mark.parametrize("log_n,log_b,D", SHAPES)
def test_proofs_are_the_reference_proofs(zk, orc, log_n, log_b, D):
    """K 1..3, coset leaves off and on; per K the two runs take complementary (hash, q, grinding), so every value occurs with
    every K.  Context.prove equals stop_ref.stop_proof in data and state, zk_verify_stop accepts it (strict too), and
    Context.final_poly() is the reference's coefficient list."""
    trace = _trace(1 << log_n)
    si = SHAPES.index((log_n, log_b, D))
    lib = zk.load()
    for K in (1, 2, 3):
        for coset in (False, True):
            bits = (si + K) ^ (7 if coset else 0)
            hash_kind, q, g = bits & 1, (1, 3)[(bits >> 1) & 1], (0, 6)[(bits >> 2) & 1]
            ref = stop_ref.stop_proof(orc, log_n, log_b, q, hash_kind, K, coset, D, g)
            with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D) as ctx:
                assert lib.zk_ctx_get_fri_stop(ctx._h) == D and lib.zk_ctx_get_early_launch(ctx._h) == 0
                p = ctx.prove(trace)
                what = (K, coset, hash_kind, q, g)
                assert len(p.data) == p.data_len() == stop_ref.proof_len(log_n, log_b, q, g, K, coset, D), what
                assert (p.data, p.state) == (ref.data, ref.state), what
                assert p.check(strict=True) == 0 and p.check() == 0, what
                out = C.c_int32(1)
                assert lib.zk_verify_stop(p.data, len(p.data), p.state, log_n, log_b, p.public_last, hash_kind, q, g, K, int(coset), D, C.byref(out)) == 0
                assert out.value == 0
                assert list(ctx.final_poly()) == ref.coef and len(ref.coef) == 1 << D, what
                info = ctx.last_transcript()
                assert info.free_term == ref.coef[0] and bytes(info.roots[1 + log_n - D]) == bytes(32)


PREFIX = b"early stop: a transcript prefix"


@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("log_n,log_b,D,K", [(6, 3, 2, 1), (10, 3, 4, 3), (10, 3, 4, 1)])
def test_host_levels_channel_and_prove_many(zk, orc, log_n, log_b, D, K, coset):
    """The same bytes with device-only trees (0, 0) and the default hand-over, through zk_prove_channel on a non-empty prefix, and
    from zk_prove_many on two contexts; the self-checks pass on the layers that exist."""
    trace = _trace(1 << log_n)
    kw = dict(fold_log=K, coset_leaves=coset, stop_log=D, queries=2)
    ref = stop_ref.stop_proof(orc, log_n, log_b, 2, 0, K, coset, D)
    refp = stop_ref.stop_proof(orc, log_n, log_b, 2, 0, K, coset, D, prefix=PREFIX)
    with zk.Context(log_n, log_b, **kw) as a, zk.Context(log_n, log_b, **kw) as b:
        b.trace_upload(trace)
        default_levels = a.host_levels
        for hl in ((0, 0), default_levels):
            a.set_host_levels(*hl)
            b.set_host_levels(*hl)
            p = a.prove(trace)
            assert (p.data, p.state) == (ref.data, ref.state), hl
            for pm in zk.prove_many([a, b]):
                assert (pm.data, pm.state) == (ref.data, ref.state), ("many", hl)
                assert pm.stop_log == D and pm.check(strict=True) == 0
            ch = zk.Channel()
            ch.commit(PREFIX)
            pc = b.prove_channel(ch)
            assert (pc.data, pc.state) == (refp.data, refp.state), ("channel", hl)
            assert pc.stop_log == D
        a.set_checks(True)
        p = a.prove(trace)
        assert (p.data, p.state) == (ref.data, ref.state)


@pytest.mark.parametrize("K,coset", [(1, False), (3, True)])
def test_switching_on_one_live_context(zk, orc, K, coset):
    """D = 0, then D = 2, then D = 0 on one context: the first and the third proof are the full format's, byte for byte; after the
    second, reads of ids past the stop answer ZK_ERR_STATE."""
    log_n, log_b, D = 10, 3, 2
    trace = _trace(1 << log_n)
    lib = zk.load()
    full = stop_ref.stop_proof(orc, log_n, log_b, 1, 0, K, coset, 0)
    if K == 1 and not coset:
        assert full.data == orc.prove(log_n, log_b).proof         # today's proof: the reference's bytes
    with zk.Context(log_n, log_b, fold_log=K, coset_leaves=coset) as ctx:
        first = ctx.prove(trace)
        assert (first.data, first.state) == (full.data, full.state) and first.stop_log == 0
        assert list(ctx.final_poly()) == [ctx.last_transcript().free_term]
        ctx.layer_read(1 + log_n)
        ctx.merkle_node(1 + log_n, 0)
        ctx.set_fri_stop(D)
        second = ctx.prove(trace)
        ref = stop_ref.stop_proof(orc, log_n, log_b, 1, 0, K, coset, D)
        assert (second.data, second.state) == (ref.data, ref.state)
        Rp = log_n - D
        assert np.array_equal(ctx.layer_read(1 + Rp), ref.c.layers[1 + Rp])    # the stopped layer is there, its tree is not
        buf, n = C.create_string_buffer(32 * 64), C.c_size_t()
        for lid in range(1 + Rp, log_n + 2):
            assert lib.zk_merkle_node(ctx._h, lid, 0, buf) == ZK_ERR_STATE, lid
            assert lib.zk_merkle_nodes(ctx._h, lid, 0, 1, buf) == ZK_ERR_STATE, lid
            assert lib.zk_merkle_path(ctx._h, lid, 0, buf, C.byref(n)) == ZK_ERR_STATE, lid
        word = np.zeros(1, dtype=np.uint32)
        for lid in range(2 + Rp, log_n + 2):
            assert lib.zk_layer_read(ctx._h, lid, 0, 1, word.ctypes.data_as(C.c_void_p)) == ZK_ERR_STATE, lid
        ctx.set_fri_stop(0)
        third = ctx.prove(trace)
        assert (third.data, third.state) == (full.data, full.state)
        ctx.layer_read(1 + log_n)
        ctx.merkle_node(1 + log_n, 0)                             # everything is materialised again


@pytest.mark.parametrize("K", [1, 3])
def test_bad_trace_fails_the_final_degree_check(zk, K):
    log_n, log_b, D = 6, 3, 2
    trace = _trace(1 << log_n).copy()
    trace[17] = (int(trace[17]) + 1) % P
    with zk.Context(log_n, log_b, fold_log=K, stop_log=D) as ctx:
        with pytest.raises(zk.ZkError) as e:
            ctx.prove(trace)
        assert e.value.code == ZK_ERR_CHECK and "final FRI layer has degree >= 2^2" in str(e.value)
        assert "trace does not satisfy the constraints" in str(e.value)
        good = ctx.prove(_trace(1 << log_n))                      # the context is fine afterwards
        assert good.check(strict=True) == 0


def test_limits(zk):
    lib = zk.load()
    with zk.Context(6, 3) as ctx:
        ctx.set_fri_stop(5)
        assert lib.zk_ctx_set_fri_stop(ctx._h, 6) == ZK_ERR_INVALID and lib.zk_ctx_get_fri_stop(ctx._h) == 5      # D = log_n
        ctx.set_fri_stop(0)
        assert lib.zk_ctx_get_fri_stop(ctx._h) == 0
    with zk.Context(10, 3, stop_log=3) as ctx:
        assert lib.zk_ctx_set_fri_stop(ctx._h, 9) == ZK_ERR_INVALID and lib.zk_ctx_get_fri_stop(ctx._h) == 3      # D = 9
        assert lib.zk_ctx_set_fri_stop(ctx._h, 8) == 0 and lib.zk_ctx_get_fri_stop(ctx._h) == 8
    with zk.Context(10, 5, stop_log=7) as ctx:
        assert lib.zk_ctx_set_fri_stop(ctx._h, 8) == ZK_ERR_INVALID and lib.zk_ctx_get_fri_stop(ctx._h) == 7      # D + log_b = 13
        with pytest.raises(zk.ZkError):
            ctx.set_fri_stop(8)
        assert ctx.stop_log == 7
    assert lib.zk_ctx_set_fri_stop(None, 1) == ZK_ERR_INVALID and lib.zk_ctx_get_fri_stop(None) == 0
