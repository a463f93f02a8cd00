"""The one-call prover with challenges in E = F_P[u] / (u^2 - 5) (zk_ctx_set_ext, Context(ext_log=1)) on the GPU: every proof
is the one tests/ext_ref.py builds without the library -- bytes, final state, public_last, the component-1 raws of the challenges and
every node of every committed tree -- and the CPU verifier accepts it strictly; one live context walked ext 0 -> 1 -> 0 -> 1 with the other
settings changing in between; zk_prove_many over an ext and a plain context; a broken trace; the setter against a running proof."""
import ctypes as C
import threading

import numpy as np
import pytest

import cap_ref
import ext_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_CHECK = -1, -4, -7

# (log_n, log_b, q, hash, K, coset, D, cap, grinding bits, host levels): chosen so that every value of every setting appears with every size
# class it can take (D = 2 needs log_n >= 3), every K with both leaf formats, and host levels default / off / (1, 0) with SHA-256
SETTINGS = [
    (2, 1, 1, 0, 1, False, 0, 0, 0, None), (2, 1, 16, 1, 2, True, 0, 4, 8, None), (2, 1, 1, 0, 1, True, 0, 8, 0, (0, 0)),
    (2, 1, 1, 0, 2, False, 0, 0, 0, (1, 0)),
    (4, 2, 1, 0, 1, True, 0, 4, 0, None), (4, 2, 16, 1, 1, False, 2, 0, 8, None), (4, 2, 1, 1, 2, False, 0, 8, 0, None),
    (4, 2, 16, 0, 2, True, 2, 4, 0, (0, 0)), (4, 2, 1, 0, 3, False, 2, 4, 8, (1, 0)), (4, 2, 16, 0, 3, True, 0, 8, 0, None),
    (4, 2, 1, 0, 3, False, 0, 0, 0, (0, 0)), (4, 2, 1, 1, 3, True, 2, 0, 0, None),
    (10, 3, 1, 0, 1, False, 0, 4, 0, None), (10, 3, 1, 1, 1, True, 2, 0, 0, None), (10, 3, 1, 0, 2, False, 2, 8, 8, None),
    (10, 3, 1, 1, 2, True, 0, 0, 0, None), (10, 3, 1, 1, 3, False, 0, 8, 0, None), (10, 3, 1, 0, 3, True, 2, 4, 8, None),
    (10, 3, 16, 0, 1, False, 0, 0, 0, (0, 0)), (10, 3, 1, 0, 3, True, 0, 0, 0, (1, 0)), (10, 3, 16, 0, 3, False, 2, 0, 0, None),
    (10, 3, 1, 0, 1, True, 0, 0, 8, (0, 0)), (10, 3, 1, 0, 2, True, 2, 8, 0, (1, 0)), (10, 3, 1, 0, 3, True, 0, 0, 0, None),
]


def test_every_value_of_every_setting_appears():
    assert len(SETTINGS) == 24 and len(set(SETTINGS)) == 24
    assert {(s[4], s[5]) for s in SETTINGS} == {(k, c) for k in (1, 2, 3) for c in (False, True)}
    assert {s[6] for s in SETTINGS} == {0, 2} and {s[7] for s in SETTINGS} == {0, 4, 8} and {s[8] for s in SETTINGS} == {0, 8}
    for size in ((2, 1), (4, 2), (10, 3)):                    # per size: both hashes, both query counts, all three host-level settings
        mine = [s for s in SETTINGS if s[:2] == size]
        assert {s[3] for s in mine} == {0, 1} and {s[2] for s in mine} == {1, 16} and {s[9] for s in mine} == {None, (0, 0), (1, 0)}, size
        assert {s[5] for s in mine} == {False, True} and {s[4] for s in mine} >= {1, 2}, size
    for size in ((4, 2), (10, 3)):
        mine = [s for s in SETTINGS if s[:2] == size]
        assert {(s[4], s[5]) for s in mine} == {(k, c) for k in (1, 2, 3) for c in (False, True)} and {s[6] for s in mine} == {0, 2}, size


def _trace(zk, log_n, a1=3141592):
    return zk.trace_fibsq((1 << log_n) - 1, 1, a1)


def _assert_proof(zk, ctx, pr, ref, tag):
    assert pr.ext_log == 1
    assert pr.data == ref.data, tag
    assert pr.state == ref.state and pr.public_last == ref.public_last, tag
    cm = ref.c
    info = ctx.last_transcript()
    grp = ext_ref.groups(ctx.log_n - ctx.stop_log, ctx.fold_log)
    assert list(info.alpha_raw) == cm.alphas[0::2], tag
    assert [info.beta_raw[r0] for r0, _ in grp] == [cm.betas[r0][0] for r0, _ in grp], tag
    assert ctx.ext_challenges() == cm.alphas[1::2] + [cm.betas[r0][1] for r0, _ in grp], tag
    assert list(ctx.final_poly()) == list(cm.coef), tag
    assert pr.check(strict=True) == 0 and pr.check() == 0, tag
    for tid, heap in cm.trees.items():                        # every node the prover builds: from the cap's depth down
        first = (1 << cm.ce[tid]) - 1
        steps = cm.lg[0] - max(tid - 1, 0) - cm.lg[tid] if tid else 0
        got = ctx.merkle_nodes(tid, first, len(heap) - first, coset_steps=steps)
        assert np.array_equal(got, heap[first:]), (tag, tid)


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(str(v).replace(" ", "") for v in s))
def test_proofs_are_the_models_byte_for_byte(zk, orc, setting):
    log_n, log_b, q, h, K, coset, D, c, bits, levels = setting
    ref = ext_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, bits)
    with zk.Context(log_n, log_b, hash=HASH_NAMES[h], queries=q, host_levels=levels, grind_bits=bits, fold_log=K, coset_leaves=coset, stop_log=D,
                    cap_log=c, ext_log=1) as ctx:
        assert zk.load().zk_ctx_get_ext(ctx._h) == 1
        _assert_proof(zk, ctx, ctx.prove(_trace(zk, log_n)), ref, setting)
        ctx.set_checks(True)                                  # the degree checks on both planes pass on a true trace, and change nothing
        assert ctx.prove().data == ref.data


def test_one_live_context_walked_through_ext_and_back(zk, orc):
    log_n, log_b = 10, 3
    lib = zk.load()
    walk = [(0, 1, False, 0, 0), (1, 3, True, 2, 4), (0, 2, True, 0, 8), (1, 1, False, 0, 0), (1, 2, False, 2, 8), (0, 3, False, 2, 0), (1, 3, True, 0, 4)]
    with zk.Context(log_n, log_b, queries=2) as ctx:
        ctx.trace_upload(_trace(zk, log_n))
        for ext, K, coset, D, c in walk:
            ctx.set_fold(K)
            ctx.set_coset_leaves(coset)
            ctx.set_fri_stop(D)
            ctx.set_merkle_cap(c)
            ctx.set_ext(ext)
            assert lib.zk_ctx_get_ext(ctx._h) == ext
            if ext:
                _assert_proof(zk, ctx, ctx.prove(), ext_ref.proof(orc, log_n, log_b, 2, 0, K, coset, D, c), (ext, K, coset, D, c))
            else:
                ref = cap_ref.proof(orc, log_n, log_b, 2, 0, K, coset, D, c)
                pr = ctx.prove()
                assert pr.ext_log == 0 and pr.data == ref.data and pr.state == ref.state, (ext, K, coset, D, c)
                assert ctx.ext_challenges() == []
    # zk_ctx_device_bytes with ext off is what it was before the first set_ext(1), whatever was set in between
    with zk.Context(log_n, log_b, fold_log=3) as ctx:
        base = ctx.device_bytes
        ctx.set_ext(1)
        grown = ctx.device_bytes
        ctx.set_fold(1)
        ctx.set_fold(3)
        ctx.set_ext(0)
        assert grown > base and ctx.device_bytes == base
        ctx.set_ext(0)
        assert ctx.device_bytes == base


def test_prove_many_over_an_ext_and_a_plain_context(zk, orc):
    log_n, log_b = 10, 3
    with zk.Context(log_n, log_b, fold_log=2, coset_leaves=True, ext_log=1) as a, zk.Context(log_n, log_b, fold_log=2, coset_leaves=True) as b:
        for ctx in (a, b):
            ctx.trace_upload(_trace(zk, log_n))
        pa, pb = zk.prove_many([a, b])
        ea, eb = ext_ref.proof(orc, log_n, log_b, 1, 0, 2, True, 0, 0), cap_ref.proof(orc, log_n, log_b, 1, 0, 2, True, 0, 0)
        assert pa.ext_log == 1 and pa.data == ea.data and pa.state == ea.state
        assert pb.ext_log == 0 and pb.data == eb.data and pb.state == eb.state
        assert pa.check(strict=True) == 0 and pb.check(strict=True) == 0


@pytest.mark.parametrize("D", [0, 2])
def test_a_broken_trace_fails_the_check(zk, D):
    log_n, log_b = 6, 2
    trace = _trace(zk, log_n).copy()
    trace[17] ^= 1
    with zk.Context(log_n, log_b, stop_log=D, ext_log=1) as ctx:
        with pytest.raises(zk.ZkError) as e:
            ctx.prove(trace)
        assert e.value.code == ERR_CHECK
        ctx.prove(_trace(zk, log_n)).verify(strict=True)      # and the context is usable afterwards


def test_refusals(zk):
    lib = zk.load()
    with zk.Context(4, 2) as ctx:
        assert lib.zk_ctx_set_ext(ctx._h, 2) == ERR_INVALID and b"ext_log" in lib.zk_last_error()
        assert lib.zk_ctx_set_ext(None, 1) == ERR_INVALID
        ctx.set_ext(1)
        assert lib.zk_ctx_set_hash(ctx._h, 2) == ERR_INVALID
        assert b"ext_log" in lib.zk_last_error() and b"BLAKE2s" in lib.zk_last_error()
        ctx.set_ext(0)
        assert lib.zk_ctx_set_hash(ctx._h, 2) == 0
        assert lib.zk_ctx_set_ext(ctx._h, 1) == ERR_INVALID
        assert b"ext_log" in lib.zk_last_error() and b"BLAKE2s" in lib.zk_last_error()
        assert lib.zk_ctx_get_ext(ctx._h) == 0 and lib.zk_ctx_get_ext(None) == 0


def test_the_setter_is_refused_while_a_proof_runs(zk, orc):
    """prove on one thread, zk_ctx_set_ext(1) on another: the setter is refused with ZK_ERR_STATE or succeeds between two proofs (a proof that
    meets the setter is refused the same way), and every proof made is its own model's."""
    lib = zk.load()
    log_n, log_b = 10, 3
    ref = ext_ref.proof(orc, log_n, log_b, 1, 0, 1, False, 0, 0)
    with zk.Context(log_n, log_b, ext_log=1) as ctx:
        ctx.trace_upload(_trace(zk, log_n))
        proofs, errors = [], []

        def run():
            for _ in range(6):
                try:
                    proofs.append(ctx.prove())
                except zk.ZkError as e:
                    errors.append(e.code)

        t = threading.Thread(target=run)
        t.start()
        codes = []
        while t.is_alive() and len(codes) < 200:
            codes.append(lib.zk_ctx_set_ext(ctx._h, 1))
        t.join()
        assert set(codes) <= {0, ERR_STATE} and set(errors) <= {ERR_STATE}, (codes, errors)
        for p in proofs:
            assert p.data == ref.data and p.state == ref.state
        assert proofs or errors
