"""The prover tail every folding factor shares (zkstark.hip: prove_finish; batch.hip: the decommit loop; transcript.hpp:
for_each_opening, Channel::commit_group) on live contexts that change their settings in place: the free term, grinding, the
query draw, the gather list and the reused commit buffer must follow (K, queries, grind bits, hash) from one proof to the next."""
import pytest

import fold_ref
import verify_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
SEED = 3141592
# (K, queries, grind bits): up in all three, back to K = 1 with the larger tuples' buffer, a short last group, home again
SETTINGS = [(1, 1, 0), (3, 2, 8), (1, 2, 8), (2, 1, 0), (1, 1, 0)]


# (7, 1): K = 3 gives groups 3 + 3 + 1 on a 2-value last layer, K = 2 a short last group
@pytest.mark.parametrize("log_n,log_b", [(5, 2), (7, 1)])
def test_one_context_reconfigured_in_place(zk, orc, log_n, log_b):
    from zkstark_amd._lib import check
    lib = zk.load()
    trace = zk.trace_fibsq((1 << log_n) - 1, 1, SEED)
    with zk.Context(log_n, log_b) as ctx:
        for hash_kind in (0, 1):
            check(lib.zk_ctx_set_hash(ctx._h, hash_kind))
            ctx.hash = HASH_NAMES[hash_kind]
            for K, q, g in SETTINGS:
                check(lib.zk_ctx_set_queries(ctx._h, q))
                check(lib.zk_ctx_set_grinding(ctx._h, g))
                ctx.queries, ctx.grind_bits = q, g
                ctx.set_fold(K)
                p = ctx.prove(trace)
                ref = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, g)
                assert p.data == ref.data, (hash_kind, K, q, g)
                assert p.state == ref.state and p.public_last == ref.public_last, (hash_kind, K, q, g)
                if K == 1 and g == 0:                              # the oracle's own prover, where it can express the settings
                    data, state, last = verify_corpus.oracle_proofs(orc, log_n, log_b, q, hash_kind)[0]
                    assert (p.data, p.state, p.public_last) == (data, state, last), (hash_kind, q)


def test_one_batch_reconfigured_in_place(zk):
    """4 proofs at (5, 2) with 2 queries and 8 grind bits, K = 1 then 3 then 1 on one BatchContext: every proof is zk_prove's from
    a context with the same settings."""
    log_n, log_b, q, g = 5, 2, 2, 8
    a1s = [SEED + p for p in range(4)]
    with zk.BatchContext(log_n, log_b, 2, queries=q, grind_bits=g) as bc, zk.Context(log_n, log_b, queries=q, grind_bits=g) as ctx:
        bc.gen_fibsq([1] * 4, a1s)
        for K in (1, 3, 1):
            bc.set_fold(K)
            ctx.set_fold(K)
            got = bc.prove()
            for p, a1 in zip(got, a1s):
                want = ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, a1))
                assert p.data == want.data and p.state == want.state and p.public_last == want.public_last, (K, a1)
                assert p.fold_log == K and p.check(strict=True) == 0
    assert len({p.data for p in got}) == 4
