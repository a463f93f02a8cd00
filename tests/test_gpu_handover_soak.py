"""Soak of the hand-overs with ALTERNATING inputs under load, every byte against the CPU oracle.

A hand-over here is a value one workgroup (or the device) stores and another workgroup (or the host) reads without a kernel
boundary in between: the node per workgroup that merkle_wg_kernel's last workgroup carries on from (publish_node /
load_digest_agent), the 2^top digests and the layer values it posts to the host mailbox, the openings fetch_kernel returns through
host-mapped memory, the nonces of grind_kernel's mailbox, and the constant an early-launched fold reads from a pinned host slot.
The older soaks prove one trace over and over, so a consumer that reads what the PREVIOUS run left at the address reads the right
bytes.  Every case here runs two inputs in turn on the same buffers (A, B, A, B, ...): a stale read is then a wrong byte, and every
run is compared with the oracle's result for its own input (orc.prove, tests/fold_ref.py, tests/grind_ref.py, orc.merkle_build).
While a case runs, tests/handover_soak.py's load generator proves 2^22-point traces on two more host threads (SHA-256 and the
field hash, one context and stream each), back to back ("uniform") or with seeded pauses of 0 .. 2 ms ("uneven"), and checks its
own proofs too.  tests/test_handover_soak_grid.py shows on the CPU that the rows reach the hand-overs they are here for.

Measured on the MI355X (one run of this module, 16 host cores; a case's two reference proofs are inside its time, and are shared
with the cases of the same prover setting): the whole module 129 s for 68 cases, 1.9 s for the load generator's set-up, and per case,
uniform / uneven load:
  whole proofs (2 x pairs proofs each): (10, 3) 2.2 - 2.5 / 1.8 - 2.0 s for 1 000 - 2 000 proofs; (13, 3) 2.3 - 2.5 / 1.8 - 2.0 s for
    760 - 1 300; (15, 3) 2.2 - 2.3 / 1.6 - 1.8 s for 500 - 800; (17, 3) 2.3 - 2.5 / 1.5 - 2.0 s for 320 - 520; early launch 2.0 and 2.4 /
    1.5 s; fold_log 3 2.3 - 2.6 / 1.2 - 2.0 s for 600 - 1 600; grind_bits 14 2.1 / 1.7 s for 1 600;
  every node: 2^12 and 2^13 SHA-256 1.1 - 1.4 / 0.9 - 2.1 s for 2 400 and 5 000 builds; 2^16 interleaved 1.7 / 1.6 s for 2 000; 2^17
    1.3 / 1.5 s for 1 300; (19, 19, 0, 0) 1.8 / 1.7 s for 250; the field hash 2.0 / 1.9 - 2.4 s for 4 800 (2^13) and 1 800 (2^16) builds;
  batches: 2.1 / 1.2 - 1.3 s (fold_log 1) and 1.5 / 0.8 s (fold_log 3) for 2 x 200 batches; the grinder's relaunch 0.5 / 0.4 s for 20.
The counts (tests/handover_soak.py) are the floors -- 50 pairs up to N = 2^16, 30 above, 30 pairs of builds, 20 grinding batches --
scaled to about 2 s per case from a first run at the floors' order.
"""
import ctypes as C
import struct
import time

import numpy as np
import pytest

import fold_ref
import grind_ref
import handover_soak as hs
import merkle_plans as mp
from test_gpu_merkle_plans import GUARD_NODES, Dev, Heaps, assert_nodes, interleave, latency_log, words_to_nodes

pytestmark = pytest.mark.gpu

P = 3221225473


@pytest.fixture(scope="module")
def load(zk):
    gen = hs.Load(zk)
    try:
        yield gen
    finally:
        gen.close()


@pytest.fixture(scope="module")
def heaps(orc):
    return Heaps(orc)


@pytest.fixture(scope="module")
def dev(zk):
    d = Dev(zk)
    d.check(d.lib.zk_dev_set_profiling(0))            # no events around the launches under test
    try:
        yield d
    finally:
        d.close()


class Ref:
    """A reference proof: what the prover must produce, byte for byte."""

    def __init__(self, data, state):
        self.data, self.state = bytes(data), bytes(state)


_refs = {}


def reference(orc, log_n, log_b, h, q, fold_log, grind_bits, a1):
    """orc.prove, or the library-free proof of tests/fold_ref.py / tests/grind_ref.py; computed once per setting and seed."""
    key = (log_n, log_b, h, q, fold_log, grind_bits, a1)
    if key not in _refs:
        if fold_log != 1:
            r = fold_ref.fold_proof(orc, log_n, log_b, q, h, fold_log, grind_bits, a1)
            _refs[key] = Ref(r.data, r.state)
        elif grind_bits:
            data, state, _, _ = grind_ref.grind_proof(orc, log_n, log_b, q, h, grind_bits, a1=a1)
            _refs[key] = Ref(data, state)
        else:
            orc.set_queries(q)
            orc.set_hash(h)
            try:
                r = orc.prove(log_n, log_b, 1, a1, want_vectors=False)
            finally:
                orc.set_queries(1)
                orc.set_hash(orc.HASH_SHA256)
            assert r.rc == 0
            _refs[key] = Ref(r.proof, r.state)
    return _refs[key]


def finish(load, problems, what, kind, runs, t0):
    """After the load threads are joined: the case's own mismatch and the load's, in one assertion."""
    print(f"soak-time {what} {kind}: {runs} runs in {time.perf_counter() - t0:.2f} s, {load.proofs} load proofs so far")
    problems = list(problems) + list(load.errors)
    assert not problems, "\n".join(problems)


# ---- 2. whole proofs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hs.LOADS)
@pytest.mark.parametrize("row", hs.PROOF_ROWS, ids=lambda r: r.id)
def test_alternating_proofs_equal_the_oracle(zk, orc, load, dev, row, kind):
    """One context, trace_upload before every proof, traces A and B in turn; every proof.data and proof.state against the
    reference of that trace.  A mismatch names the row, the iteration, the load, the first differing byte and the root or opening
    it falls in."""
    t0 = time.perf_counter()
    layout = (row.log_n, row.log_b, row.q, row.grind_bits, row.fold_log)
    n = 1 << row.log_n
    seeds = (hs.SEED_A, hs.SEED_B)
    wants = [reference(orc, *row.ref_key, a1) for a1 in seeds]
    assert wants[0].data != wants[1].data
    traces = [zk.trace_fibsq(n - 1, 1, a1) for a1 in seeds]
    problems, runs = [], 0
    with zk.Context(row.log_n, row.log_b, hash=hs.HASH_NAMES[row.h], queries=row.q, host_levels=row.host_levels, grind_bits=row.grind_bits,
                    fold_log=row.fold_log) as ctx:
        if row.early and not ctx.set_early_launch(True):
            pytest.skip("the device has no stream memory operations")
        if row.host_levels is None and row.h == mp.SHA and zk.host_hash_mode() != "portable":
            assert ctx.host_levels == hs.DEFAULT_HOST_LEVELS                  # what the CPU-side reach assertions assume
        with latency_log(dev, row.lat if row.lat != mp.LATENCY_LOG else 0), load.running(kind, seed=len(row.id)):
            for it in range(2 * row.pairs):
                ctx.trace_upload(traces[it & 1])
                got = ctx.prove()
                runs += 1
                if got.data != wants[it & 1].data or got.state != wants[it & 1].state:
                    problems.append(hs.describe_mismatch(row.id, it, kind, got, wants[it & 1], layout))
                    break
                if load.failed.is_set():
                    break
            ctx.sync()
    finish(load, problems, row.id, kind, runs, t0)


# ---- 3. every node, the lines warm -----------------------------------------------------------------------------------------------
def leaves_b(log_m):
    v = np.random.default_rng(5150 + hs.LEAF_SEED_B + log_m).integers(0, P, size=1 << log_m, dtype=np.uint64).astype(np.uint32)
    v[0] = P - 1
    v[-1] = 0
    return v


def node_words(nodes):
    """[nodes, 32] digest bytes -> the heap's state words, as the device stores them."""
    return np.ascontiguousarray(nodes).view(">u4").astype(np.uint32).ravel()


@pytest.mark.parametrize("kind", hs.LOADS)
@pytest.mark.parametrize("h,log_m,lat,top,log_parts,pairs", hs.COMMIT_CASES,
                         ids=[f"{hs.HASH_NAMES[c[0]]}-" + "-".join(map(str, c[1:5])) for c in hs.COMMIT_CASES])
def test_alternating_commits_every_node(zk, orc, load, dev, heaps, h, log_m, lat, top, log_parts, pairs, kind):
    """zk_dev_merkle_commit into ONE heap, poisoned once, from two leaf arrays in turn; after every build the whole heap, the guard
    region and the root (which the host reduces from the posted digests) against the oracle heap of that leaf array.  A side stream
    keeps summing the heap, so every die's L2 and the CUs' vector caches keep taking in its lines with plain loads while the builds
    write them; the load generator runs as well."""
    if top and zk.host_hash_mode() == "portable":
        pytest.skip("no host hand-over on this CPU")
    t0 = time.perf_counter()
    torch = dev.torch
    what = f"{hs.HASH_NAMES[h]} commit 2^{log_m} lat {lat} top {top} parts 2^{log_parts}"
    vals = [Heaps.leaves(log_m), leaves_b(log_m)]
    want_nodes = [heaps.build(h, v) for v in vals]
    want_words = [node_words(w) for w in want_nodes]
    assert not np.array_equal(want_words[0], want_words[1])
    srcs = [dev.upload(interleave(v, log_parts)) for v in vals]
    t, poison = dev.poisoned(log_m)
    n_words = 8 * len(want_nodes[0])
    assert len(poison) == n_words + 8 * GUARD_NODES
    root = C.create_string_buffer(32)
    dev.check(dev.lib.zk_committer_set_top(dev.k, top))
    side = torch.cuda.Stream(device=dev.device)
    side.wait_stream(torch.cuda.current_stream(dev.device))
    bad, runs = None, 0
    with latency_log(dev, lat), load.running(kind, seed=log_m):
        for it in range(2 * pairs):
            with torch.cuda.stream(side):
                for _ in range(3):
                    t.sum()                                                    # discarded: the reads are the point
            dev.check(dev.lib.zk_dev_merkle_commit(dev.k, srcs[it & 1].data_ptr(), log_parts, log_m - log_parts, t.data_ptr(), dev.stream(), h, root))
            dev.sync()
            words = t.cpu().numpy().view(np.uint32)
            runs += 1
            if root.raw != bytes(want_nodes[it & 1][0]) or not np.array_equal(words[:n_words], want_words[it & 1]) or \
                    not np.array_equal(words[n_words:], poison[n_words:]):
                bad = (it, root.raw, words.copy())
                break
            if load.failed.is_set():
                break
        side.synchronize()
    dev.check(dev.lib.zk_committer_set_top(dev.k, 8 if zk.host_hash_mode() != "portable" else 0))
    problems = []
    if bad:
        it, got_root, words = bad
        where = f"{what}: build {it} (leaf set {'AB'[it & 1]}) under {kind} load"
        try:
            assert np.array_equal(words[n_words:], poison[n_words:]), f"{where}: the guard region after the heap was written"
            assert_nodes(words_to_nodes(words[:n_words]), want_nodes[it & 1], where)
            assert got_root == bytes(want_nodes[it & 1][0]), f"{where}: every node in the heap is right, the root returned to the host is not"
        except AssertionError as e:
            problems.append(str(e))
    finish(load, problems, what, kind, runs, t0)


# ---- 4. the batch prover -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", hs.LOADS)
@pytest.mark.parametrize("fold_log", [1, 3])
@pytest.mark.parametrize("h", [mp.SHA, mp.FIELD], ids=["sha256", "field"])
def test_alternating_batches_equal_the_one_call_reference(zk, orc, load, h, fold_log, kind):
    """(a) Two batch contexts prove two a1 lists in turn; every proof of every batch against orc.prove / fold_ref.fold_proof."""
    t0 = time.perf_counter()
    problems, runs = [], 0
    what = f"batch {hs.HASH_NAMES[h]} fold {fold_log}"
    for log_n, log_b, log_batch in hs.BATCH_ROWS:
        batch = 1 << log_batch
        lists = [hs.batch_a1s(k, batch) for k in (0, 1)]
        wants = [[reference(orc, log_n, log_b, h, 1, fold_log, 0, a1) for a1 in a1s] for a1s in lists]
        layout = (log_n, log_b, 1, 0, fold_log)
        with zk.BatchContext(log_n, log_b, log_batch, hash=hs.HASH_NAMES[h], fold_log=fold_log) as bc, load.running(kind, seed=log_n):
            for it in range(2 * hs.BATCH_PAIRS[(log_n, log_b, log_batch)]):
                bc.gen_fibsq([1] * batch, lists[it & 1])
                data, states = bc.prove_raw()
                runs += 1
                for p, want in enumerate(wants[it & 1]):
                    got = Ref(data[p].tobytes(), states[p].tobytes())
                    if got.data != want.data or got.state != want.state:
                        problems.append(hs.describe_mismatch(f"{what} ({log_n}, {log_b}) x 2^{log_batch}, proof {p}", it, kind, got, want, layout))
                if problems or load.failed.is_set():
                    break
        if problems or load.errors:
            break
    finish(load, problems, what, kind, runs, t0)


@pytest.mark.parametrize("kind", hs.LOADS)
def test_alternating_batches_that_relaunch_the_grinder(zk, orc, load, kind):
    """(b) g = 12 on 64 proofs: in both lists some proofs' smallest nonce lies beyond the first launch's 2^14 nonces, so grind_device
    launches again for them alone and compacts its job table (tests/test_handover_soak_grid.py re-derives that from grind_ref).
    Every nonce and every proof of 20 batches against grind_ref."""
    t0 = time.perf_counter()
    log_n, log_b, log_batch, g = hs.GRIND_BATCH
    batch = 1 << log_batch
    refs = [[grind_ref.grind_proof(orc, log_n, log_b, 1, 0, g, a1=a1) for a1 in a1s] for a1s in hs.GRIND_LISTS]
    for k in (0, 1):
        assert hs.grind_conditions([r[3] for r in refs[k]]) == (True, True, True)
    off = grind_ref.prefix_len(log_n)
    problems, runs = [], 0
    with zk.BatchContext(log_n, log_b, log_batch, grind_bits=g) as bc, load.running(kind, seed=g):
        for it in range(hs.GRIND_BATCHES):
            bc.gen_fibsq([1] * batch, hs.GRIND_LISTS[it & 1])
            data, states = bc.prove_raw()
            runs += 1
            for p, (want_data, want_state, _, want_nonce) in enumerate(refs[it & 1]):
                got = Ref(data[p].tobytes(), states[p].tobytes())
                nonce = struct.unpack("<Q", got.data[off:off + 8])[0]
                if nonce != want_nonce:
                    problems.append(f"grinding batch {it} (list {'AB'[it & 1]}) under {kind} load: proof {p} has nonce {nonce}, the smallest is {want_nonce}")
                elif got.data != want_data or got.state != want_state:
                    problems.append(hs.describe_mismatch(f"grinding batch, proof {p}", it, kind, got, Ref(want_data, want_state), (log_n, log_b, 1, g, 1)))
            if problems or load.failed.is_set():
                break
    finish(load, problems, "grinding batch", kind, runs, t0)
