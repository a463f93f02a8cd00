"""One live batch and one live batched verifier walked through every pair of their settings (tests/batch_walk.py; DESIGN.md 7d
"Reconfiguring a live context"): after the setters of the factors that changed, every proof of the next zk_batch_prove -- or the one
proof of the next zk_batch_prove_shared -- is the reference proof of the new configuration byte for byte, every tree the batch hands out
is this proof's node for node from its cap down or answers ZK_ERR_STATE, the device bytes follow D and the pinned cap buffer alone, a
failed proof in between leaves nothing behind, refused setters change nothing, and the verifier's verdicts on the proofs and on mutated
copies are the CPU verifier's."""
import ctypes as C

import numpy as np
import pytest

import batch_walk as bw
import cap_ref
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
    if _changed(prev, step, "cap"):
        bc.set_merkle_cap(step.cap)
    if _changed(prev, step, "rows"):                          # also between two zk_batch_prove steps, which do not look at it
        bc.set_shared_rows(step.rows)
    if _changed(prev, step, "host"):
        assert lib.zk_batch_set_host_levels(bc._h, step.host) == 0
    if _changed(prev, step, "threads"):
        assert lib.zk_batch_set_threads(bc._h, step.threads) == 0


def _configure_verifier(lib, v, step, prev, log_batch):
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
    if _changed(prev, step, "cap"):
        v.set_merkle_cap(step.cap)
    if prev is not None and bw.verifier_shared(prev, log_batch) != bw.verifier_shared(step, log_batch):
        v.set_shared(*bw.verifier_shared(step, log_batch))
    assert (lib.zk_verifier_get_shared(v._h), lib.zk_verifier_get_shared_rows(v._h)) == tuple(map(int, bw.verifier_shared(step, log_batch)))


def _check_tree(lib, orc, bc, t, heaps, caps, ce, log_m, width, log_n, log_batch, hash_kind, what):
    """Batch tree `t`, built with leaves of 2^width values over 2^log_m leaves per proof and committed at depth ce: proof p's share is
    heaps[p] node for node from the cap's depth down, its cap is caps[p], the heap is as long as this leaf width makes it, and (ce > 0)
    the node in front of the caps was built by no one."""
    nb = 1 << log_batch
    heap_len = 2 * (nb << log_m) - 1
    one = C.create_string_buffer(32)
    assert lib.zk_batch_merkle_nodes(bc._h, t, heap_len - 1, 1, one) == 0, (what, "last node of tree", t)        # the heap of THIS leaf width:
    assert lib.zk_batch_merkle_nodes(bc._h, t, heap_len, 1, one) == ZK_ERR_INVALID, (what, "one past tree", t)   # no shorter, no longer
    assert lib.zk_batch_merkle_cap_log(bc._h, t) == ce == min(bc.cap_log, log_m - 1), (what, "cap depth of tree", t)
    for p in range(nb):
        assert bc.merkle_cap(t, p).tobytes() == caps[p], (what, "cap of tree", t, "proof", p)
    first = (1 << (log_batch + ce)) - 1                       # where the caps begin
    if ce:
        assert lib.zk_batch_merkle_nodes(bc._h, t, first - 1, 1, one) == ZK_ERR_STATE, (what, "above the cap of tree", t)
    if log_batch == 0:                                        # the one-call prover behind the batch: the root or the cap, through the same call
        if ce == 0:
            assert bytes(bc.merkle_nodes(t, 0, 1, coset_steps=width)[0]) == bytes(heaps[0][0]), (what, "root", t)
        else:
            assert bc.merkle_nodes(t, first, 1 << ce, coset_steps=width).tobytes() == caps[0], (what, "cap level", t)
        return
    depths = log_m if log_n <= FULL_TREES_UP_TO else min(log_m, DEPTHS_ABOVE)
    if ce == 0:
        first = 0                                             # roots are committed: the call hashes the levels above them itself
    heap = bc.merkle_nodes(t, first, min(heap_len, (1 << (log_batch + depths + 1)) - 1) - first, coset_steps=width)
    for p in range(nb):
        assert len(heaps[p]) == (2 << log_m) - 1, (what, "tree", t)
        for dd in range(ce, depths + 1):
            at = (1 << (log_batch + dd)) - 1 + (p << dd) - first
            assert np.array_equal(heap[at:at + (1 << dd)], heaps[p][(1 << dd) - 1:(2 << dd) - 1]), (what, "tree", t, "proof", p, "depth", dd)
    if ce == 0:
        orc.set_hash(hash_kind)                               # above the per-proof roots: one heap over the whole batch
        try:
            for i in range(nb - 2, -1, -1):
                assert bytes(heap[i]) == orc.node_hash(bytes(heap[2 * i + 1]), bytes(heap[2 * i + 2])), (what, "tree", t, "node", i)
        finally:
            orc.set_hash(0)


def _answers_state(lib, bc, t, what):
    """Tree `t` is not the last proof's: both read-outs say so (a success could only be an earlier proof's nodes)."""
    one, cap = C.create_string_buffer(32), C.create_string_buffer(32 << cap_ref.MAX_CAP)
    assert lib.zk_batch_merkle_nodes(bc._h, t, 0, 1, one) == ZK_ERR_STATE, (what, "tree", t)
    return lib.zk_batch_merkle_cap(bc._h, t, 0, cap, len(cap)) == ZK_ERR_STATE


def _check_readouts(lib, orc, bc, refs, step, log_n, log_b, log_batch, what):
    """Step 4: every tree id of 0 .. log_n + 1 is this proof's, node for node under the leaf width it was built with from its cap down,
    or ZK_ERR_STATE."""
    L = log_n + log_b
    widths = bw.tree_steps(log_n, step)
    if step.call == "shared":                                 # tree 0 is every statement's f tree, or (rows) the one tree over the rows
        cm = refs[0].c
        if not step.rows:
            caps = [cap_ref.cap_of(tree, cm.ce[0]) for tree in cm.f_trees]
            _check_tree(lib, orc, bc, 0, cm.f_trees, caps, cm.ce[0], L, 0, log_n, log_batch, step.hash, what)
        for t in range(0 if step.rows else 1, log_n + 2):
            assert _answers_state(lib, bc, t, what), (what, "cap of tree", t)
        return
    assert all(set(r.c.trees) == set(widths) for r in refs), what
    one = C.create_string_buffer(32)
    for t in range(log_n + 2):
        if t not in widths:                                   # a success here could only be an earlier proof's nodes
            assert lib.zk_batch_merkle_nodes(bc._h, t, 0, 1, one) == ZK_ERR_STATE, (what, "tree", t)
            assert _answers_state(lib, bc, t, what), (what, "cap of tree", t)
            continue
        log_m = (L if t == 0 else L - (t - 1)) - widths[t]   # leaves of one proof's tree
        assert all(r.c.lg[t] == log_m and r.c.ce[t] == refs[0].c.ce[t] for r in refs), (what, "tree", t)
        _check_tree(lib, orc, bc, t, [r.c.trees[t] for r in refs], [r.c.caps[t] for r in refs], refs[0].c.ce[t], log_m, widths[t], log_n, log_batch,
                    step.hash, what)


def _mutations(shape, i, proofs):
    """[(proof index, bytes)] of step i's three one-bit mutations."""
    out = []
    for p, byte, bit in bw.bit_flips(shape, i, len(proofs), len(proofs[0].data)):
        data = bytearray(proofs[p].data)
        data[byte] ^= 1 << bit
        out.append((p, bytes(data)))
    return out


def _check_verifier(zk, v, proofs, shape, i, step, what):
    """Step 6 after zk_batch_prove: the proofs pass, strict and plain; with three one-bit mutations added, every verdict is the CPU
    verifier's."""
    log_n, log_b = shape
    for strict in (True, False):
        got = v.verify(proofs, strict=strict)
        assert len(got) == len(proofs) and not got.any(), (what, strict, got)
    muts = [zk.Proof(proofs[p].state, data, log_n, log_b, proofs[p].public_last, HASH_NAMES[step.hash], step.q, step.bits, step.K, step.coset,
                     step.D, step.cap) for p, data in _mutations(shape, i, proofs)]
    for strict in (True, False):
        got = v.verify(list(proofs) + muts, strict=strict).tolist()
        want = [p.check(strict=strict) for p in list(proofs) + muts]
        assert got == want, (what, strict, got, want)
        assert got[-1] != 0, (what, strict, "a flipped path digest was accepted")


def _shared_copy(zk, sp, data=None, public_last=None):
    return zk.SharedProof(sp.state, sp.data if data is None else data, sp.log_n, sp.log_blowup, sp.log_batch,
                          sp.public_last if public_last is None else public_last, sp.hash, sp.queries, sp.grind_bits, sp.fold_log, sp.coset_leaves,
                          sp.stop_log, sp.cap_log, sp.shared_rows)


def _check_verifier_shared(zk, v, sp, shape, i, what):
    """Step 6 after zk_batch_prove_shared: the proof five times in one run, strict and plain; then with three one-bit mutations and one
    copy whose first and last statement have swapped their public inputs, every verdict the CPU verifier's."""
    for strict in (True, False):
        got = v.verify([sp] * 5, strict=strict)
        assert len(got) == 5 and not got.any(), (what, strict, got)
    muts = [_shared_copy(zk, sp, data=data) for _, data in _mutations(shape, i, [sp])]
    last = np.array(sp.public_last, dtype=np.uint32)
    last[0], last[-1] = sp.public_last[-1], sp.public_last[0]
    assert last[0] != last[-1]
    swapped = _shared_copy(zk, sp, public_last=last)
    for strict in (True, False):
        got = v.verify([sp] * 5 + muts + [swapped], strict=strict).tolist()
        want = [p.check(strict=strict) for p in [sp] * 5 + muts + [swapped]]
        assert got == want, (what, strict, got, want)
        assert got[7] != 0, (what, strict, "a flipped path digest was accepted")
        assert got[8] != 0, (what, strict, "swapped public inputs were accepted")


def _check_plain_proof_under_shared_settings(zk, orc, v, sp, shape, step, what):
    """Once per walk, right after the verifier has changed to shared proofs: a plain proof of the same settings, zero-padded to the shared
    length, gets the CPU verifier's number for the shared settings, and that number is not 0."""
    plain = bw.expected(orc, shape, step._replace(call="each"), 0)
    assert len(plain.data) < len(sp.data) == v.proof_len, what
    data = np.zeros((1, v.proof_len), dtype=np.uint8)
    data[0, :len(plain.data)] = np.frombuffer(plain.data, dtype=np.uint8)
    for strict in (True, False):
        states = np.frombuffer(plain.state, dtype=np.uint8).reshape(1, 32) if strict else None
        got = int(v.verify_raw(data, np.array(sp.public_last, dtype=np.uint32).reshape(1, -1), states)[0])
        padded = _shared_copy(zk, sp, data=data[0].tobytes())
        padded.state = plain.state
        assert got == padded.check(strict=strict) != 0, (what, strict, got)


def _refused_setters(lib, bc, v, prev, log_batch, what):
    """Step 7: five setters with arguments out of range answer ZK_ERR_INVALID and leave every setting as it was."""
    assert lib.zk_batch_set_merkle_cap(bc._h, 9) == ZK_ERR_INVALID, what
    assert lib.zk_verifier_set_merkle_cap(v._h, 9) == ZK_ERR_INVALID, what
    assert lib.zk_verifier_set_shared(v._h, 9, 0) == ZK_ERR_INVALID, what
    assert lib.zk_verifier_set_shared(v._h, 0, 1) == ZK_ERR_INVALID, what
    assert lib.zk_batch_set_hash(bc._h, 2) == ZK_ERR_INVALID, what
    assert lib.zk_batch_get_merkle_cap(bc._h) == prev.cap, what
    assert (lib.zk_verifier_get_shared(v._h), lib.zk_verifier_get_shared_rows(v._h)) == tuple(map(int, bw.verifier_shared(prev, log_batch))), what


@pytest.mark.parametrize("log_n,log_b,log_batch", [(7, 2, 2), (10, 3, 1), (6, 2, 0), (7, 2, 3)])
def test_walk_on_one_live_batch(zk, orc, log_n, log_b, log_batch):
    """(7, 2, 2): four proofs, host-built levels, one workgroup of the final-polynomial kernel for all proofs, cap 8 at depth 10 of the
    batch heap, which the mailbox just holds; (10, 3, 1): layers of up to 2048 values at the stop and the deepest trees; (6, 2, 0): a
    batch of one forwards every setter to a zk_ctx and refuses shared proofs; (7, 2, 3): eight proofs, cap 8 at depth 11: the post kernel
    and the pinned buffer."""
    lib, shape, nb, n = zk.load(), (log_n, log_b), 1 << log_batch, 1 << log_n
    steps = bw.walk(log_n, log_b, log_batch >= 1)
    assert len(steps) <= bw.MAX_STEPS
    faults = bw.fault_steps(steps, bw.fault_kinds(log_batch >= 1))
    assert steps[0]._replace(host=1, threads=16, entry="gen_fibsq", seeds="A") == bw.FRESH
    traces = {name: np.stack([zk.trace_fibsq(n - 1, 1, base + p) for p in range(nb)]) for name, base in bw.SEED_SETS.items()}
    spot = 100 if n - 1 > 100 else n // 2                     # the trace value a fault step corrupts (a trace of 2^6 - 1 values has no index 100)
    const_bytes = None                                        # device bytes without the final-polynomial tables, once d_work exists
    shared_seen = False
    try:
        with zk.BatchContext(log_n, log_b, log_batch) as bc, zk.Verifier(log_n, log_b) as v:
            fresh_bytes = bc.device_bytes
            prev = None
            for i, step in enumerate(steps):
                what = (i, tuple(step))
                if i == len(steps) // 2:                      # in the middle of the walk: this step proves and verifies as if they had not been called
                    _refused_setters(lib, bc, v, prev, log_batch, what)
                _configure_batch(lib, bc, step, prev)
                assert (lib.zk_batch_get_merkle_cap(bc._h), lib.zk_batch_get_shared_rows(bc._h)) == (step.cap, int(step.rows)), what
                shared = step.call == "shared"
                refs = [bw.expected(orc, shape, step, p, log_batch) for p in range(1 if shared else nb)]
                if log_batch == 0 and step.rows:              # a batch of one makes no shared proof, and the refusal leaves nothing behind
                    with pytest.raises(zk.ZkError) as e:
                        bc.prove_shared()
                    assert e.value.code == ZK_ERR_INVALID, (what, str(e.value))
                if i in faults:                               # a proof that fails, in this configuration, before the good one
                    broken = bw.broken_proofs(steps, i, log_batch)
                    bad = traces[step.seeds].copy()
                    for p in broken:
                        bad[p, spot] = (int(bad[p, spot]) + 1) % P
                    bc.set_traces(bad)
                    with pytest.raises(zk.ZkError) as e:
                        bc.prove_shared() if shared else bc.prove()
                    assert e.value.code == ZK_ERR_CHECK, (what, str(e.value))
                    assert bw.fault_message(step) in str(e.value) and bw.fault_culprit(step, broken) in str(e.value), (what, str(e.value))
                if step.entry == "gen_fibsq":
                    bc.gen_fibsq(*bw.seeds_of(step, nb))
                else:
                    bc.set_traces(traces[step.seeds])
                plen = bw.expected_len(shape, step, log_batch)
                if shared:
                    sp = bc.prove_shared()
                    ref = refs[0]
                    assert (sp.data, sp.state, [int(x) for x in sp.public_last]) == (ref.data, ref.state, ref.public_last), what
                    assert sp.check(strict=True) == 0, what
                    assert len(sp.data) == plen == lib.zk_proof_data_len_shared_rows(log_n, log_b, step.q, step.bits, step.K, int(step.coset), step.D,
                                                                                   step.cap, log_batch, int(step.rows)), what
                else:
                    proofs = bc.prove()
                    if step.cap == 0:
                        assert plen == stop_ref.proof_len(log_n, log_b, step.q, step.bits, step.K, step.coset, step.D), what
                    assert len(proofs) == nb and bc.proof_len == plen, what
                    for p, (got, ref) in enumerate(zip(proofs, refs)):
                        assert (got.data, got.state, got.public_last) == (ref.data, ref.state, ref.public_last), (what, "proof", p)
                        assert len(got.data) == plen and got.check(strict=True) == 0, (what, "proof", p)
                assert (lib.zk_batch_get_fold(bc._h), lib.zk_batch_get_coset_leaves(bc._h), lib.zk_batch_get_fri_stop(bc._h)) \
                    == (step.K, int(step.coset), step.D), what
                assert (lib.zk_batch_get_merkle_cap(bc._h), lib.zk_batch_get_shared_rows(bc._h)) == (step.cap, int(step.rows)), what
                _check_readouts(lib, orc, bc, refs, step, log_n, log_b, log_batch, what)
                if log_batch:                                 # step 5: d_work comes once and stays, the final-polynomial tables follow D,
                    tables = nb * ((1 << step.D) + 1) * 4 if step.D else 0           # the pinned cap buffer follows the cap; call and rows change nothing
                    pinned = 4 * bw.pinned_cap_words(log_n, log_b, log_batch, step.cap)
                    assert (pinned > 0) == ((log_n, log_b, log_batch, step.cap) == (7, 2, 3, 8)), what
                    if const_bytes is None and sw.fmt(step) != bw.PLAIN:
                        const_bytes = bc.device_bytes - tables - pinned
                        assert const_bytes == fresh_bytes + 32 * nb, what       # include/zkstark_amd.h: 32 bytes per proof
                    assert bc.device_bytes == (fresh_bytes if const_bytes is None else const_bytes) + tables + pinned, what
                _configure_verifier(lib, v, step, prev, log_batch)
                if shared:
                    if not shared_seen:
                        _check_plain_proof_under_shared_settings(zk, orc, v, sp, shape, step, what)
                        shared_seen = True
                    _check_verifier_shared(zk, v, sp, shape, i, what)
                else:
                    _check_verifier(zk, v, proofs, shape, i, step, what)
                prev = step
            assert shared_seen == (log_batch >= 1)
    finally:
        bw.forget_commits()
