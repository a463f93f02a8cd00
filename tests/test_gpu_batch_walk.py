"""One live batch and one live batched verifier walked through every pair of their settings (tests/batch_walk.py; DESIGN.md 7d
"Reconfiguring a live context"): after the setters of the factors that changed, every proof of the next zk_batch_prove is the reference
proof of the new configuration byte for byte, every tree the batch hands out is this proof's node for node or answers ZK_ERR_STATE, the
device bytes follow D alone, a failed zk_batch_prove in between leaves nothing behind, and the verifier's verdicts on the proofs and on
three mutated copies are the CPU verifier's."""
import ctypes as C

import numpy as np
import pytest

import batch_walk as bw
import settings_walk as sw
import stop_ref
from transforms_ref import P

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ZK_ERR_INVALID, ZK_ERR_STATE, ZK_ERR_CHECK = -1, -4, -7
FULL_TREES_UP_TO = 7                                         # log_n <= 7: every node; above: depths 0 .. DEPTHS_ABOVE of every proof's tree
DEPTHS_ABOVE = 9                                             # ... every host-built level (at most 8 per proof) and one device level below


def _changed(prev, step, f):
    return prev is not None and getattr(prev, f) != getattr(step, f)


def _configure_batch(lib, bc, step, prev):
    """The setters of the factors that differ from `prev`; none on step 0 (the fresh batch is bw.FRESH)."""
    if _changed(prev, step, "hash"):
        assert lib.zk_batch_set_hash(bc._h, step.hash) == 0
        bc.hash = HASH_NAMES[step.hash]
    if _changed(prev, step, "q"):
        assert lib.zk_batch_set_queries(bc._h, step.q) == 0
        bc.queries = step.q
    if _changed(prev, step, "bits"):
        assert lib.zk_batch_set_grinding(bc._h, step.bits) == 0
        bc.grind_bits = step.bits
    if _changed(prev, step, "K"):
        bc.set_fold(step.K)
    if _changed(prev, step, "coset"):
        bc.set_coset_leaves(step.coset)
    if _changed(prev, step, "D"):
        bc.set_fri_stop(step.D)
    if _changed(prev, step, "host"):
        assert lib.zk_batch_set_host_levels(bc._h, step.host) == 0
    if _changed(prev, step, "threads"):
        assert lib.zk_batch_set_threads(bc._h, step.threads) == 0


def _configure_verifier(lib, v, step, prev):
    if _changed(prev, step, "hash"):
        assert lib.zk_verifier_set_hash(v._h, step.hash) == 0
        v.hash = HASH_NAMES[step.hash]
    if _changed(prev, step, "q"):
        assert lib.zk_verifier_set_queries(v._h, step.q) == 0
        v.queries = step.q
    if _changed(prev, step, "bits"):
        assert lib.zk_verifier_set_grinding(v._h, step.bits) == 0
        v.grind_bits = step.bits
    if _changed(prev, step, "K"):
        v.set_fold(step.K)
    if _changed(prev, step, "coset"):
        v.set_coset_leaves(step.coset)
    if _changed(prev, step, "D"):
        v.set_fri_stop(step.D)


def _check_readouts(lib, orc, bc, refs, step, log_n, log_b, log_batch, what):
    """Step 3: every tree id of 0 .. log_n + 1 is this proof's, node for node under the leaf width it was built with, or ZK_ERR_STATE."""
    L, nb = log_n + log_b, 1 << log_batch
    widths = bw.tree_steps(log_n, step)
    assert all(set(r.c.trees) == set(widths) for r in refs), what
    one = C.create_string_buffer(32)
    for t in range(log_n + 2):
        if t not in widths:                                   # a success here could only be an earlier proof's nodes
            assert lib.zk_batch_merkle_nodes(bc._h, t, 0, 1, one) == ZK_ERR_STATE, (what, "tree", t)
            continue
        log_m = (L if t == 0 else L - (t - 1)) - widths[t]   # leaves of one proof's tree
        heap_len = 2 * (nb << log_m) - 1
        assert lib.zk_batch_merkle_nodes(bc._h, t, heap_len - 1, 1, one) == 0, (what, "last node of tree", t)        # the heap of THIS leaf width:
        assert lib.zk_batch_merkle_nodes(bc._h, t, heap_len, 1, one) == ZK_ERR_INVALID, (what, "one past tree", t)   # no shorter, no longer
        if log_batch == 0:                                    # the one-call prover behind the batch: the root, through the same call
            assert bytes(bc.merkle_nodes(t, 0, 1, coset_steps=widths[t])[0]) == refs[0].c.roots[t], (what, "root", t)
            continue
        depths = log_m if log_n <= FULL_TREES_UP_TO else min(log_m, DEPTHS_ABOVE)
        heap = bc.merkle_nodes(t, 0, min(heap_len, (1 << (log_batch + depths + 1)) - 1), coset_steps=widths[t])
        for p, ref in enumerate(refs):
            assert len(ref.c.trees[t]) == (2 << log_m) - 1, (what, "tree", t)
            for dd in range(depths + 1):
                at = (1 << (log_batch + dd)) - 1 + (p << dd)
                assert np.array_equal(heap[at:at + (1 << dd)], ref.c.trees[t][(1 << dd) - 1:(2 << dd) - 1]), (what, "tree", t, "proof", p, "depth", dd)
        orc.set_hash(step.hash)                               # above the per-proof roots: one heap over the whole batch
        try:
            for i in range(nb - 2, -1, -1):
                assert bytes(heap[i]) == orc.node_hash(bytes(heap[2 * i + 1]), bytes(heap[2 * i + 2])), (what, "tree", t, "node", i)
        finally:
            orc.set_hash(0)


def _check_verifier(zk, v, proofs, shape, i, step, what):
    """Step 5: the proofs pass, strict and plain; with three one-bit mutations added, every verdict is the CPU verifier's."""
    log_n, log_b = shape
    for strict in (True, False):
        got = v.verify(proofs, strict=strict)
        assert len(got) == len(proofs) and not got.any(), (what, strict, got)
    muts = []
    for p, byte, bit in bw.bit_flips(shape, i, len(proofs), len(proofs[0].data)):
        data = bytearray(proofs[p].data)
        data[byte] ^= 1 << bit
        muts.append(zk.Proof(proofs[p].state, bytes(data), log_n, log_b, proofs[p].public_last, HASH_NAMES[step.hash], step.q, step.bits,
                             step.K, step.coset, step.D))
    for strict in (True, False):
        got = v.verify(list(proofs) + muts, strict=strict).tolist()
        want = [p.check(strict=strict) for p in list(proofs) + muts]
        assert got == want, (what, strict, got, want)
        assert got[-1] != 0, (what, strict, "a flipped path digest was accepted")


@pytest.mark.parametrize("log_n,log_b,log_batch", [(7, 2, 2), (10, 3, 1), (6, 2, 0)])
def test_walk_on_one_live_batch(zk, orc, log_n, log_b, log_batch):
    """(7, 2, 2): four proofs, host-built levels, one workgroup of the final-polynomial kernel for all proofs; (10, 3, 1): layers of up
    to 2048 values at the stop and the deepest trees; (6, 2, 0): a batch of one forwards every setter to a zk_ctx."""
    lib, shape, nb, n = zk.load(), (log_n, log_b), 1 << log_batch, 1 << log_n
    steps = bw.walk(log_n, log_b)
    faults = bw.fault_steps(steps)
    assert steps[0]._replace(host=1, threads=16, entry="gen_fibsq", seeds="A") == bw.FRESH
    traces = {name: np.stack([zk.trace_fibsq(n - 1, 1, base + p) for p in range(nb)]) for name, base in bw.SEED_SETS.items()}
    spot = 100 if n - 1 > 100 else n // 2                     # the trace value a fault step corrupts (a trace of 2^6 - 1 values has no index 100)
    const_bytes = None                                        # device bytes without the final-polynomial tables, once d_work exists
    try:
        with zk.BatchContext(log_n, log_b, log_batch) as bc, zk.Verifier(log_n, log_b) as v:
            fresh_bytes = bc.device_bytes
            prev = None
            for i, step in enumerate(steps):
                what = (i, tuple(step))
                _configure_batch(lib, bc, step, prev)
                refs = [bw.expected(orc, shape, step, p) for p in range(nb)]
                if i in faults:                               # a zk_batch_prove that fails, in this configuration, before the good one
                    broken = bw.broken_proofs(steps, i, log_batch)
                    bad = traces[step.seeds].copy()
                    for p in broken:
                        bad[p, spot] = (int(bad[p, spot]) + 1) % P
                    bc.set_traces(bad)
                    with pytest.raises(zk.ZkError) as e:
                        bc.prove()
                    assert e.value.code == ZK_ERR_CHECK, (what, str(e.value))
                    assert bw.fault_message(step) in str(e.value) and f"proof {min(broken)} of the batch" in str(e.value), (what, str(e.value))
                if step.entry == "gen_fibsq":
                    bc.gen_fibsq(*bw.seeds_of(step, nb))
                else:
                    bc.set_traces(traces[step.seeds])
                proofs = bc.prove()
                plen = stop_ref.proof_len(log_n, log_b, step.q, step.bits, step.K, step.coset, step.D)
                assert len(proofs) == nb and bc.proof_len == plen, what
                for p, (got, ref) in enumerate(zip(proofs, refs)):
                    assert (got.data, got.state, got.public_last) == (ref.data, ref.state, ref.public_last), (what, "proof", p)
                    assert len(got.data) == plen and got.check(strict=True) == 0, (what, "proof", p)
                assert (lib.zk_batch_get_fold(bc._h), lib.zk_batch_get_coset_leaves(bc._h), lib.zk_batch_get_fri_stop(bc._h)) \
                    == (step.K, int(step.coset), step.D), what
                _check_readouts(lib, orc, bc, refs, step, log_n, log_b, log_batch, what)
                if log_batch:                                 # step 4: d_work comes once and stays, the final-polynomial tables follow D
                    tables = nb * ((1 << step.D) + 1) * 4 if step.D else 0
                    if const_bytes is None and sw.fmt(step) != bw.PLAIN:
                        const_bytes = bc.device_bytes - tables
                        assert const_bytes == fresh_bytes + 32 * nb, what       # include/zkstark_amd.h: 32 bytes per proof
                    assert bc.device_bytes == (fresh_bytes if const_bytes is None else const_bytes + tables), what
                _configure_verifier(lib, v, step, prev)
                _check_verifier(zk, v, proofs, shape, i, step, what)
                prev = step
    finally:
        bw.forget_commits()
