"""FRI folding factor 2^K on the GPU (zk_ctx_set_fold, zk_fri_fold_multi, zk_dev_fri_fold_multi; DESIGN.md "Folding factor"): the
multi-fold kernel against `steps` oracle folds, and every one-call prover against the proofs tests/fold_ref.py builds without the
library -- bytes, state, every committed layer and every node of every committed tree."""
import ctypes as C

import numpy as np
import pytest

import fold_ref
from transforms_ref import P, rand_field, require_memory

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_CHECK = -1, -4, -7
BETAS = (0, 1, P - 1, P + 5, 2**32 - 1)                      # the last two: raw challenges >= P


@pytest.fixture
def hb():
    from sharded_mirror import HipBackend
    b = HipBackend(0)
    yield b
    b.close()


def _trace(n, a1=3141592):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


def _dev_fold(hb, dom, layer, log_m, rnd, steps, beta, aligned):
    from zkstark_amd._lib import check
    off = 0 if aligned else 1
    src, dst = hb.empty(len(layer) + off)[off:], hb.empty((len(layer) >> steps) + off)[off:]
    assert (src.data_ptr() % 16 == 0) == aligned
    src.copy_(hb.upload(layer))
    check(hb.lib.zk_dev_fri_fold_multi(dom, src.data_ptr(), dst.data_ptr(), log_m, rnd, steps, beta, hb._stream()))
    return hb.to_host(dst)


def _rounds(log_n):
    """Every round for small domains, the ends and the middle for large ones."""
    return range(log_n) if log_n <= 7 else sorted({0, 1, 2, log_n // 2, log_n - 4, log_n - 3, log_n - 2, log_n - 1})


@pytest.mark.parametrize("log_n", [3, 4, 5, 6, 7, 10, 13, 16, 18])
def test_dev_fold_multi_matches_steps_oracle_folds(orc, hb, log_n):
    """zk_dev_fri_fold_multi at every (log_m, round, steps) of the grid -- outputs of 2 and 4 values included (log_b 1, 2 at the
    last group) -- on 16-byte aligned buffers (the 16-byte kernel) and one word past (the scalar kernel)."""
    case = 0
    for log_b in (1, 2, 3, 4):
        L = log_n + log_b
        dom = hb.domain(log_n, log_b, 5)
        rng = np.random.default_rng(100 * log_n + log_b)
        for rnd in _rounds(log_n):
            layer = rand_field(rng, 1 << (L - rnd))
            layer[0] = layer[-1] = P - 1
            for steps in (1, 2, 3):
                if rnd + steps > log_n:
                    continue
                beta = BETAS[case % len(BETAS)] if case % 3 else int(rng.integers(0, 2**32))
                want = fold_ref.fold_layer(orc, layer, log_n, log_b, rnd, steps, beta)
                for aligned in ((True, False) if L - rnd <= 14 else (bool(case & 1),)):
                    got = _dev_fold(hb, dom, layer, L - rnd, rnd, steps, beta, aligned)
                    assert np.array_equal(got, want), (log_b, rnd, steps, beta, aligned)
                case += 1


def test_dev_fold_multi_every_special_beta(orc, hb):
    log_n, log_b = 9, 3
    dom = hb.domain(log_n, log_b, 5)
    layer = rand_field(np.random.default_rng(5), 1 << (log_n + log_b - 2))
    for beta in BETAS:
        for steps in (1, 2, 3):
            for aligned in (True, False):
                got = _dev_fold(hb, dom, layer, log_n + log_b - 2, 2, steps, beta, aligned)
                assert np.array_equal(got, fold_ref.fold_layer(orc, layer, log_n, log_b, 2, steps, beta)), (beta, steps, aligned)


def test_dev_fold_multi_domain_2e26(orc, hb):
    """One shape at domain 2^26: layer 0 -> layer 3 in one pass."""
    log_n, log_b = 23, 3
    require_memory(3 * (4 << 26), 4 * (4 << 26))
    dom = hb.domain(log_n, log_b, 5, fold_only=True)
    layer = rand_field(np.random.default_rng(26), 1 << 26)
    got = _dev_fold(hb, dom, layer, 26, 0, 3, P + 77, True)
    assert np.array_equal(got, fold_ref.fold_layer(orc, layer, log_n, log_b, 0, 3, P + 77))


@pytest.mark.parametrize("log_n,log_b", [(4, 1), (5, 2), (10, 3), (13, 1), (16, 3)])
def test_ctx_fold_multi_matches_steps_oracle_folds(zk, orc, log_n, log_b):
    """zk_fri_fold_multi on context-resident layers; steps = 1 gives what zk_fri_fold gives."""
    rng = np.random.default_rng(log_n)
    with zk.Context(log_n, log_b) as ctx:
        for rnd in _rounds(log_n):
            layer = rand_field(rng, 1 << (log_n + log_b - rnd))
            for steps in (1, 2, 3):
                if rnd + steps > log_n:
                    continue
                beta = int(rng.integers(0, 2**32))
                ctx.layer_write(1 + rnd, layer)
                ctx.fri_fold_multi(rnd, steps, beta)
                got = ctx.layer_read(1 + rnd + steps)
                assert np.array_equal(got, fold_ref.fold_layer(orc, layer, log_n, log_b, rnd, steps, beta)), (rnd, steps)
                if steps == 1:
                    ctx.fri_fold(rnd, beta)
                    assert np.array_equal(ctx.layer_read(2 + rnd), got)


def _same(p, ref):
    assert p.data == ref.data, "proof bytes"
    assert p.state == ref.state and p.public_last == ref.public_last


def _check_committed(zk, ctx, ref, log_n, K):
    """Every value of every committed layer and every node of every committed tree; the ids in between: ZK_ERR_STATE."""
    info = ctx.last_transcript()
    ids = sorted(ref.c.layers)
    for i in ids:
        assert np.array_equal(ctx.layer_read(i), ref.c.layers[i]), f"layer {i}"
        assert np.array_equal(ctx.merkle_nodes(i), ref.c.trees[i]), f"tree {i}"
        assert bytes(info.roots[i]) == ref.c.roots[i]
    for r0, beta in ref.c.betas.items():
        assert info.beta_raw[r0] == beta
    assert info.free_term == ref.c.free_term and list(info.alpha_raw) == ref.c.alphas
    for i in range(log_n + 2):
        if i in ids:
            continue
        assert bytes(info.roots[i]) == bytes(32) and info.beta_raw[i - 1] == 0
        for call in (lambda: ctx.layer_read(i, 0, 1), lambda: ctx.merkle_node(i, 0), lambda: ctx.merkle_nodes(i, 0, 1), lambda: ctx.merkle_path(i, 0)):
            with pytest.raises(zk.ZkError) as e:
                call()
            assert e.value.code == ERR_STATE


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n", [4, 5, 10, 13, 16])
@pytest.mark.parametrize("K", [2, 3])
def test_one_call_prover_equals_the_reference(zk, orc, K, log_n, hash_kind):
    for log_b in (1, 3):
        for q in (1, 7):
            g = 12 if (log_n, log_b, q) == (10, 3, 7) else 0
            ref = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, g)
            datas = []
            for levels in ((0, 0), (8, 0), (8, 9)):
                with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, host_levels=levels, grind_bits=g, fold_log=K) as ctx:
                    assert ctx.set_early_launch(True) is False           # not supported with fold_log > 1: answers 0, the proof is the same
                    p = ctx.prove(_trace(1 << log_n))
                    _same(p, ref)
                    assert p.fold_log == K and p.check(strict=True) == 0 and p.check() == 0
                    if q == 1:
                        _check_committed(zk, ctx, ref, log_n, K)
                datas.append(p.data)
            assert datas[0] == datas[1] == datas[2]
            assert fold_ref.verify(orc, p.data, p.state, log_n, log_b, p.public_last, hash_kind, q, g, K) == 0


@pytest.mark.parametrize("lat", [12, 20])
def test_latency_switch_on_both_sides(zk, orc, lat):
    """The committed layers of a 2^16 domain lie above and below the level where a Merkle build turns to its latency phase."""
    from zkstark_amd import _lib
    log_n, log_b = 13, 3
    _lib.check(_lib.load().zk_dev_set_merkle_latency_log(lat))
    try:
        for K in (2, 3):
            ref = fold_ref.fold_proof(orc, log_n, log_b, 2, 0, K)
            with zk.Context(log_n, log_b, queries=2, fold_log=K) as ctx:
                _same(ctx.prove(_trace(1 << log_n)), ref)
                ctx.sync()
    finally:
        _lib.check(_lib.load().zk_dev_set_merkle_latency_log(0))


def test_k1_set_explicitly_is_the_default(zk, orc):
    for log_n, log_b, q in ((5, 2, 1), (10, 3, 3)):
        with zk.Context(log_n, log_b, queries=q) as a, zk.Context(log_n, log_b, queries=q) as b:
            b.set_fold(2)
            b.set_fold(1)
            t = _trace(1 << log_n)
            pa, pb = a.prove(t), b.prove(t)
            assert pa.data == pb.data and pa.state == pb.state
            assert pa.data == fold_ref.fold_proof(orc, log_n, log_b, q, 0, 1).data
            b.set_fold(3)                                    # ... and a context goes from one factor to another and back
            _same(b.prove(t), fold_ref.fold_proof(orc, log_n, log_b, q, 0, 3))
            b.set_fold(1)
            assert b.prove(t).data == pa.data
            assert np.array_equal(b.layer_read(2), a.layer_read(2))      # every id is materialised again


def test_prove_channel_on_a_prefixed_channel(zk, orc):
    log_n, log_b = 7, 2
    for K in (2, 3):
        for prefix in (b"", b"session 7: " + bytes(range(40))):
            ref = fold_ref.fold_proof(orc, log_n, log_b, 1, 0, K, prefix=prefix)
            with zk.Context(log_n, log_b, fold_log=K) as ctx:
                ctx.trace_upload(_trace(1 << log_n))
                ch = zk.Channel()
                if prefix:
                    ch.commit(prefix)
                p = ctx.prove_channel(ch)
            assert p.data == ref.data and p.state == ref.state and p.fold_log == K
            if not prefix:
                assert p.check(strict=True) == 0


def test_prove_many_of_mixed_k(zk, orc):
    log_n, log_b = 10, 3
    ks = (1, 2, 3, 2)
    ctxs = [zk.Context(log_n, log_b, queries=3, fold_log=K) for K in ks]
    try:
        for c in ctxs:
            c.trace_upload(_trace(1 << log_n))
        proofs = zk.prove_many(ctxs)
    finally:
        for c in ctxs:
            c.close()
    for K, p in zip(ks, proofs):
        _same(p, fold_ref.fold_proof(orc, log_n, log_b, 3, 0, K))
        assert p.check(strict=True) == 0


@pytest.mark.parametrize("K", [2, 3])
def test_checks_name_a_broken_trace(zk, K):
    log_n, log_b = 10, 3
    t = _trace(1 << log_n)
    with zk.Context(log_n, log_b, fold_log=K) as ctx:
        ctx.set_checks(True)
        assert ctx.prove(t).check(strict=True) == 0          # the degree of every committed layer is what the checks expect
        bad = t.copy()
        bad[300] = (int(bad[300]) + 1) % P
        with pytest.raises(zk.ZkError) as e:
            ctx.prove(bad)
        assert e.value.code == ERR_CHECK


@pytest.mark.parametrize("K", [3, 2])
def test_domain_2e24(zk, orc, K):
    """Domain 2^24 (log_n 21, log_b 3), SHA-256: the bytes of the reference, accepted by the strict verifier."""
    log_n, log_b = 21, 3
    require_memory(3 << 30, 6 << 30)
    ref = fold_ref.fold_proof(orc, log_n, log_b, 1, 0, K)
    fold_ref.committed.cache_clear()
    with zk.Context(log_n, log_b, fold_log=K) as ctx:
        p = ctx.prove(_trace(1 << log_n))
    assert p.data == ref.data and p.state == ref.state
    out = C.c_int32(7)
    assert zk.load().zk_verify_fold(p.data, len(p.data), p.state, log_n, log_b, p.public_last, 0, 1, 0, K, C.byref(out)) == 0 and out.value == 0


def test_argument_errors(zk, hb):
    lib = zk.load()
    with zk.Context(6, 2) as ctx:
        for K in (0, 4):
            assert lib.zk_ctx_set_fold(ctx._h, K) == ERR_INVALID
        assert lib.zk_ctx_get_fold(ctx._h) == 1
        for steps in (0, 4):
            assert lib.zk_fri_fold_multi(ctx._h, 0, steps, 1) == ERR_INVALID
        assert lib.zk_fri_fold_multi(ctx._h, 4, 3, 1) == ERR_INVALID        # rounds 4..6 of 6: one too many
        assert lib.zk_fri_fold_multi(ctx._h, 6, 1, 1) == ERR_INVALID
        assert lib.zk_fri_fold_multi(ctx._h, 3, 3, 1) == 0
        assert lib.zk_ctx_set_fold(ctx._h, 3) == 0 and lib.zk_ctx_get_fold(ctx._h) == 3
    dom = hb.domain(6, 2, 5)
    a, b = hb.empty(256), hb.empty(256)
    for steps in (0, 4):
        assert lib.zk_dev_fri_fold_multi(dom, a.data_ptr(), b.data_ptr(), 8, 0, steps, 1, hb._stream()) == ERR_INVALID
    assert lib.zk_dev_fri_fold_multi(dom, a.data_ptr(), b.data_ptr(), 4, 4, 3, 1, hb._stream()) == ERR_INVALID     # round + steps beyond R
    assert lib.zk_dev_fri_fold_multi(dom, a.data_ptr(), b.data_ptr(), 7, 0, 2, 1, hb._stream()) == ERR_INVALID     # size does not match the round
    assert lib.zk_dev_fri_fold_multi(dom, a.data_ptr(), b.data_ptr(), 8, 0, 2, 1, hb._stream()) == 0
    hb.sync()
