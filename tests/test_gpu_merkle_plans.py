"""Every node of every Merkle launch plan against the CPU oracle (merkle.rs:14-51), byte for byte.

The root of a tree is the one value the proofs pin; the other nodes leave merkle_wg_kernel / merkle_subtree_kernel through
separate stores in every form (tests/merkle_plans.py names the forms).  So every case here compares the whole heap:
  - device-buffer builds (zk_dev_merkle_build_ex, zk_dev_merkle_commit with and without a host top and with interleaved
    leaves, zk_dev_merkle_build_chunk + the finish pass) into a buffer poisoned before the build, with a guard region after it;
    the grid is chosen by the planner mirror (tests/test_merkle_plans.py: it reaches every form), and each case's launches and
    algorithmic bytes per kernel class are checked against what the mirror predicts;
  - the trees of a context and of a batch after a proof of a SECOND trace, so that a node that is no longer stored still holds
    the first trace's value and fails.
BLAKE2s (its throughput kernel is a copy, not an instance, of merkle_subtree_kernel) is held to hashlib.blake2s
(tests/blake2s_ref.py) in the same way: the plain build on the same grid, and -- the committer and the chunk builds refuse the
hash -- the plans with a counter through a context's stand-alone commitments, with and without coset leaves.
"""
import ctypes as C

import blake2s_ref
import merkle_plans as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 3221225473
HASH_NAMES = {mp.SHA: "sha256", mp.FIELD: "field", mp.B2S: "blake2s"}
HASH_OF = {name: h for h, name in HASH_NAMES.items()}
MERKLE_CLASSES = ("merkle_leaf", "merkle_inner", "merkle_top")
GUARD_NODES = 64


class Heaps:
    """Oracle heaps over the grid's leaves, one per (hash, log_m), kept for the cases that share them.  The oracle's hash is
    selected per heap and set back to SHA-256 afterwards.  The oracle has no BLAKE2s: those heaps are hashlib's
    (blake2s_ref.tree), over leaves that are any 32-bit word, 0 and 0xffffffff among them."""

    def __init__(self, orc):
        self.orc, self.cache = orc, {}

    @staticmethod
    def leaves(log_m, h=mp.SHA):
        top = 1 << 32 if h == mp.B2S else P
        v = np.random.default_rng(5150 + log_m).integers(0, top, size=1 << log_m, dtype=np.uint64).astype(np.uint32)
        v[0] = 0
        v[-1] = top - 1
        return v

    def build(self, h, vals, steps=0):
        """steps: coset leaves of 2^steps values (BLAKE2s only here)."""
        if h == mp.B2S:
            return blake2s_ref.tree(vals, steps)
        assert steps == 0
        self.orc.set_hash(h)
        try:
            return self.orc.merkle_build(vals)
        finally:
            self.orc.set_hash(self.orc.HASH_SHA256)

    def get(self, h, log_m):
        key = (h, log_m)
        if key not in self.cache:
            if len(self.cache) >= 6:
                self.cache.pop(min(self.cache, key=lambda k: k[1]))      # keep the big ones: the grid revisits them
            self.cache[key] = self.build(h, self.leaves(log_m, h))
        return self.cache[key]


@pytest.fixture(scope="module")
def heaps(orc):
    return Heaps(orc)


class Dev:
    """The zk_dev_* Merkle entry points on torch device tensors (as tests/sharded_mirror.py), with the Merkle kernel classes
    profiled and a committer."""

    def __init__(self, zk):
        import torch
        from zkstark_amd import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.device = torch.device("cuda", 0)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(99)
        self.k = C.c_void_p()
        self.check(self.lib.zk_committer_create(0, C.byref(self.k)))
        self.check(self.lib.zk_dev_set_profiling(sum(1 << _lib.KERNEL_CLASSES.index(c) for c in MERKLE_CLASSES)))
        self.stats()

    def check(self, rc):
        self._lib.check(rc)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def sync(self):
        self.torch.cuda.current_stream(self.device).synchronize()

    def upload(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).to(self.device)

    def poisoned(self, log_m):
        """A heap of 2^(log_m+1) - 1 nodes and GUARD_NODES more, filled with random words; returns (tensor, host copy)."""
        words = ((2 << log_m) - 1 + GUARD_NODES) * 8
        t = self.torch.randint(-2**31, 2**31 - 1, (words,), dtype=self.torch.int32, device=self.device, generator=self.gen)
        return t, t.cpu().numpy().view(np.uint32)

    def stats(self):
        arr = self._lib.kernel_stat_array()
        self.check(self.lib.zk_dev_kernel_stats(arr, len(arr), 1))
        return {name: (int(a.launches), a.bytes) for name, a in zip(self._lib.KERNEL_CLASSES, arr) if name in MERKLE_CLASSES}

    def close(self):
        self.sync()
        self.lib.zk_dev_set_profiling(0)
        self.stats()
        self.lib.zk_committer_destroy(self.k)


@pytest.fixture(scope="module")
def dev(zk):
    d = Dev(zk)
    try:
        yield d
    finally:
        d.close()


class latency_log:
    """zk_dev_set_merkle_latency_log for one case (process-wide): the default is restored after the stream has drained."""

    def __init__(self, dev, lat):
        self.dev, self.lat = dev, lat

    def __enter__(self):
        self.dev.check(self.dev.lib.zk_dev_set_merkle_latency_log(self.lat))

    def __exit__(self, *exc):
        self.dev.sync()
        self.dev.check(self.dev.lib.zk_dev_set_merkle_latency_log(0))


def words_to_nodes(words):
    """Heap state words (8 per node) -> [nodes, 32] digest bytes, as zk_merkle_node gives them."""
    return np.ascontiguousarray(words).reshape(-1, 8).astype(">u4").view(np.uint8).reshape(-1, 32)


def depth_of(i):
    return int(i + 1).bit_length() - 1


def assert_nodes(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} nodes differ; first at heap index " + \
        ", ".join(f"{i} (depth {depth_of(i)})" for i in bad[:6])


def check_heap(t, poison, want, what, written=None):
    """The heap in t equals `want` where `written` (default: everywhere) and still holds the poison elsewhere and in the guard."""
    n = len(want)
    words = t.cpu().numpy().view(np.uint32)
    assert np.array_equal(words[8 * n:], poison[8 * n:]), f"{what}: the guard region after the heap was written"
    got = words_to_nodes(words[:8 * n])
    if written is not None:
        want = np.where(written[:, None], want, words_to_nodes(poison[:8 * n]))
    assert_nodes(got, want, what)


def check_profile(dev, launches, what):
    want = mp.profile(launches)
    got = dev.stats()
    assert got == {c: want.get(c, (0, 0.0)) for c in MERKLE_CLASSES}, f"{what}: the library ran another plan than the mirror's"


def interleave(vals, log_parts):
    """All-to-all order: leaf u*parts + q at recv[q*cnt + u]."""
    return np.ascontiguousarray(vals.reshape(-1, 1 << log_parts).T).ravel()


# ---- device-buffer entry points -------------------------------------------------------------------------------------------
def cases(fn, hashes=(mp.SHA, mp.FIELD)):
    return [pytest.param(h, *c, id=f"{HASH_NAMES[h]}-" + "-".join(map(str, c))) for h in hashes for c in fn(h)]


@pytest.mark.parametrize("h,log_m,lat", cases(mp.build_cases, (mp.SHA, mp.FIELD, mp.B2S)))
def test_build_ex_every_node(zk, dev, heaps, h, log_m, lat):
    """zk_dev_merkle_build_ex: no counter, so the latency phase runs plain launches of <= 10 levels (Merkle.new's plan)."""
    vals = dev.upload(Heaps.leaves(log_m, h))
    t, poison = dev.poisoned(log_m)
    with latency_log(dev, lat):
        dev.stats()
        dev.check(dev.lib.zk_dev_merkle_build_ex(vals.data_ptr(), log_m, t.data_ptr(), dev.stream(), h))
        dev.sync()
        check_profile(dev, mp.plan(log_m, h, counter=False, lat=lat), f"build 2^{log_m} lat {lat}")
    check_heap(t, poison, heaps.get(h, log_m), f"build 2^{log_m} lat {lat}")


@pytest.mark.parametrize("h,log_m,lat,top,log_parts", cases(mp.commit_cases))
def test_commit_every_node(zk, dev, heaps, h, log_m, lat, top, log_parts):
    """zk_dev_merkle_commit: the plan every proof runs (a counter: one launch with a continuation), the host top, and leaves
    in all-to-all order (log_parts > 0)."""
    if top and zk.host_hash_mode() == "portable":
        pytest.skip("no host hand-over on this CPU")
    want = heaps.get(h, log_m)
    log_parts = min(log_parts, log_m)
    src = dev.upload(interleave(Heaps.leaves(log_m), log_parts))
    t, poison = dev.poisoned(log_m)
    root = C.create_string_buffer(32)
    dev.check(dev.lib.zk_committer_set_top(dev.k, top))
    what = f"commit 2^{log_m} lat {lat} top {top} parts 2^{log_parts}"
    with latency_log(dev, lat):
        dev.stats()
        dev.check(dev.lib.zk_dev_merkle_commit(dev.k, src.data_ptr(), log_parts, log_m - log_parts, t.data_ptr(), dev.stream(), h, root))
        dev.sync()
        eff_top = top if h == mp.SHA and log_m > top else 0           # zk_dev_merkle_commit: the field hash builds to the root
        check_profile(dev, mp.plan(log_m, h, counter=True, top=eff_top, lat=lat), what)
    assert root.raw == bytes(want[0]), what
    check_heap(t, poison, want, what)


@pytest.mark.parametrize("h,log_m,log_chunks,lat,log_parts,top", cases(mp.chunk_cases))
def test_chunk_builds_every_node(zk, dev, heaps, h, log_m, log_chunks, lat, log_parts, top):
    """zk_dev_merkle_build_chunk for each chunk in turn -- each writes its own range of the heap and nothing else -- then
    zk_dev_merkle_finish (top None) or zk_dev_merkle_commit_finish."""
    if top and zk.host_hash_mode() == "portable":
        pytest.skip("no host hand-over on this CPU")
    want = heaps.get(h, log_m)
    vals = Heaps.leaves(log_m)
    log_sub = log_m - log_chunks
    log_parts = min(log_parts, log_sub)
    low = mp.chunk_handover_depth(log_m, log_chunks, lat)              # the chunk builds write depths low .. log_m
    t, poison = dev.poisoned(log_m)
    written = np.zeros(len(want), dtype=bool)
    what = f"chunks 2^{log_m} / 2^{log_chunks} lat {lat} parts 2^{log_parts}"
    with latency_log(dev, lat):
        # zk_dev_merkle_commit_finish: the field hash builds to the root on the device
        chunks, fin = mp.chunk_plans(log_m, log_chunks, h, lat, counter=top is not None, top=top if top and h == mp.SHA else 0)
        dev.stats()
        for c in range(1 << log_chunks):
            recv = dev.upload(interleave(vals[c << log_sub:(c + 1) << log_sub], log_parts))
            dev.check(dev.lib.zk_dev_merkle_build_chunk(recv.data_ptr(), log_parts, log_sub - log_parts, t.data_ptr(), log_m, c, dev.stream(), h))
            dev.sync()
            check_profile(dev, chunks[c], f"{what} chunk {c}")
            for d in range(low, log_m + 1):
                w = 1 << (d - log_chunks)
                written[(1 << d) - 1 + c * w:(1 << d) - 1 + (c + 1) * w] = True
            check_heap(t, poison, want, f"{what} after chunk {c}", written)
        if top is None:
            dev.check(dev.lib.zk_dev_merkle_finish(t.data_ptr(), log_m, log_chunks, dev.stream(), h))
        else:
            root = C.create_string_buffer(32)
            dev.check(dev.lib.zk_committer_set_top(dev.k, top))
            dev.check(dev.lib.zk_dev_merkle_commit_finish(dev.k, t.data_ptr(), log_m, log_chunks, dev.stream(), h, root))
            assert root.raw == bytes(want[0]), what
        dev.sync()
        check_profile(dev, fin, f"{what} finish")
    check_heap(t, poison, want, f"{what} after the finish")


# ---- context trees -----------------------------------------------------------------------------------------------------------
TRACE_A, TRACE_B = 3141592, 2718281


@pytest.mark.parametrize("hash_name,log_n,log_b,host_levels,early,q", [
    ("sha256", 2, 1, None, False, 1),
    ("sha256", 6, 2, (0, 0), False, 1),
    ("sha256", 10, 3, (8, 9), True, 7),
    ("sha256", 10, 3, (5, 6), False, 1),
    ("sha256", 12, 3, (10, 9), False, 7),
    ("sha256", 13, 3, (0, 0), True, 1),        # 2^16 leaves: below the latency switch
    ("sha256", 15, 3, (8, 9), False, 1),       # 2^18: throughput launches first
    ("sha256", 15, 3, (10, 9), True, 7),
    ("field", 6, 2, None, False, 1),
    ("field", 10, 3, None, True, 7),
    ("field", 13, 3, None, False, 1),
    ("field", 15, 3, None, True, 1),
    ("blake2s", 2, 1, None, False, 1),
    ("blake2s", 6, 2, None, False, 1),
    ("blake2s", 10, 3, None, True, 7),
    ("blake2s", 13, 3, None, False, 1),
    ("blake2s", 14, 3, None, True, 7),         # 2^17 leaves: the largest tree the latency kernel takes alone; the fused fold trees
                                               # below it run every continuation split from 2^16 down
    ("blake2s", 15, 3, None, False, 1),        # 2^18: a throughput launch first
])
def test_context_trees_every_node_after_a_second_trace(zk, orc, heaps, monkeypatch, hash_name, log_n, log_b, host_levels, early, q):
    """Every node of trees 0 .. R+1 after proofs of trace A then trace B on one context (the host top and tail, early launch,
    several queries): a node the second proof fails to store keeps trace A's value.  A BLAKE2s proof is verified by
    zk_verify_stop, whatever its settings: the strict verification at the end must get there."""
    h = HASH_OF[hash_name]
    n = 1 << log_n
    lib = zk.load()
    real_verify_stop, stop_calls = lib.zk_verify_stop, []
    monkeypatch.setattr(lib, "zk_verify_stop", lambda *a: (stop_calls.append(a[6]), real_verify_stop(*a))[1])
    with zk.Context(log_n, log_b, hash=hash_name, queries=q, host_levels=host_levels) as ctx:
        if early:
            on = ctx.set_early_launch(True)
            assert on or h != mp.B2S, "the gate stayed off: the BLAKE2s launches behind it would not run"
        ctx.prove(zk.trace_fibsq(n - 1, 1, TRACE_A))
        proof = ctx.prove(zk.trace_fibsq(n - 1, 1, TRACE_B))
        for tr in range(log_n + 2):
            assert_nodes(ctx.merkle_nodes(tr), heaps.build(h, ctx.layer_read(tr)), f"{hash_name} ({log_n}, {log_b}) tree {tr}")
        assert [bytes(ctx.merkle_nodes(tr, 0, 1)[0]) for tr in range(log_n + 2)] == \
            [bytes(r) for r in ctx.last_transcript().roots[:log_n + 2]]
    proof.verify(strict=True)
    assert stop_calls == ([mp.B2S] if h == mp.B2S else [])


@pytest.mark.parametrize("hash_name,log_n,log_b", [("sha256", 10, 3), ("sha256", 15, 3), ("field", 10, 3), ("field", 14, 3)])
def test_context_stage_commit_every_node(zk, orc, heaps, hash_name, log_n, log_b):
    """The stage-by-stage path: lde, merkle_commit(0), then every node of tree 0 (after a whole proof of another trace)."""
    h = HASH_OF[hash_name]
    n = 1 << log_n
    with zk.Context(log_n, log_b, hash=hash_name) as ctx:
        ctx.prove(zk.trace_fibsq(n - 1, 1, TRACE_A))
        ctx.trace_upload(zk.trace_fibsq(n - 1, 1, TRACE_B))
        ctx.lde()
        root = ctx.merkle_commit(0)
        want = heaps.build(h, ctx.layer_read(0))
        assert root == bytes(want[0])
        assert_nodes(ctx.merkle_nodes(0), want, f"{hash_name} stage commit ({log_n}, {log_b})")


def context_shape(log_m):
    """(log_n, log_blowup) of the context whose layer 0 has 2^log_m values (log_m >= 3; n = 8 is refused, the blow-up is 2 .. 32)."""
    log_b = 3 if log_m >= 7 or log_m == 5 else 2 if log_m in (4, 6) else 1
    return log_m - log_b, log_b


def context_profile(ctx):
    return {c: (v["launches"], v["bytes"]) for c, v in ctx.kernel_stats().items() if c in MERKLE_CLASSES}


def staged_layer0(zk, ctx, log_n):
    """A whole proof of trace A, then trace B up to its layer 0, with the Merkle classes profiled from there on."""
    n = 1 << log_n
    ctx.prove(zk.trace_fibsq(n - 1, 1, TRACE_A))
    ctx.trace_upload(zk.trace_fibsq(n - 1, 1, TRACE_B))
    ctx.set_profiling(MERKLE_CLASSES)
    ctx.lde()
    ctx.kernel_stats()


@pytest.mark.parametrize("log_m,lat", [pytest.param(*c, id="-".join(map(str, c))) for c in mp.context_cases(mp.B2S) + mp.B2S_RAISED_CASES])
def test_blake2s_context_commit_runs_the_predicted_plan(zk, dev, heaps, log_m, lat):
    """Whole BLAKE2s trees with a counter (the continuation; only a context reaches it for this hash): merkle_commit(0) on a layer of
    2^log_m values runs the launches and bytes the mirror predicts -- the bytes of a latency launch depend on its split -- and every
    node is hashlib's, after a whole proof of another trace."""
    log_n, log_b = context_shape(log_m)
    what = f"blake2s context commit 2^{log_m} lat {lat}"
    with latency_log(dev, lat), zk.Context(log_n, log_b, hash="blake2s") as ctx:
        staged_layer0(zk, ctx, log_n)
        root = ctx.merkle_commit(0)
        want_profile = mp.profile(mp.plan(log_m, mp.B2S, counter=True, lat=lat))
        assert context_profile(ctx) == {c: want_profile.get(c, (0, 0.0)) for c in MERKLE_CLASSES}, f"{what}: the library ran another plan than the mirror's"
        want = heaps.build(mp.B2S, ctx.layer_read(0))
        assert root == bytes(want[0]), what
        assert_nodes(ctx.merkle_nodes(0), want, what)


@pytest.mark.parametrize("steps,log_m,lat", [pytest.param(*c, id="-".join(map(str, c))) for c in mp.coset_cases(mp.B2S)])
def test_blake2s_context_coset_commit_runs_the_predicted_plan(zk, dev, heaps, steps, log_m, lat):
    """BLAKE2s trees with coset leaves: merkle_commit(0, coset_steps) is one coset_leaf_hash_kernel<2, steps> launch, then the inner-mode
    build with a counter -- below a switch at 2^12 a throughput launch of k = 1 .. 4 levels first, then the latency kernel in inner mode
    with a continuation.  Profile and every node, as above."""
    log_len = log_m + steps
    log_n, log_b = context_shape(log_len)
    what = f"blake2s context coset commit 2^{log_m} leaves of 2^{steps} lat {lat}"
    with latency_log(dev, lat), zk.Context(log_n, log_b, hash="blake2s") as ctx:
        staged_layer0(zk, ctx, log_n)
        root = ctx.merkle_commit(0, coset_steps=steps)
        want_profile = mp.profile(mp.plan(log_m, mp.B2S, counter=True, lat=lat, leaf_mode=False))
        assert "merkle_leaf" not in want_profile                   # inner mode: the only leaf launch is the coset one
        want_profile["merkle_leaf"] = (1, 4.0 * float(1 << log_len) + 32.0 * float(1 << log_m))
        assert context_profile(ctx) == {c: want_profile.get(c, (0, 0.0)) for c in MERKLE_CLASSES}, f"{what}: the library ran another plan than the mirror's"
        want = heaps.build(mp.B2S, ctx.layer_read(0), steps)
        assert root == bytes(want[0]), what
        assert_nodes(ctx.merkle_nodes(0, coset_steps=steps), want, what)


def test_bulk_node_reads_agree_and_refuse_bad_ranges(zk, orc):
    """zk_merkle_nodes: any sub-range equals zk_merkle_node node by node; out-of-range arguments are refused as zk_merkle_node
    refuses them, and an empty range at the end is allowed."""
    with zk.Context(6, 2) as ctx:
        ctx.prove(zk.trace_fibsq(63))
        m = ctx.layer_size(0)
        part = ctx.merkle_nodes(0, 100, 37)
        assert [bytes(x) for x in part] == [ctx.merkle_node(0, i) for i in range(100, 137)]
        assert ctx.merkle_nodes(0, 2 * m - 1, 0).shape == (0, 32)
        for tree, first, count in ((0, 2 * m - 1, 1), (0, 0, 2 * m), (0, 2 * m, 0), (6 + 2, 0, 1), (1, 2 * m - 2, 2)):
            with pytest.raises(zk.ZkError):
                ctx.merkle_nodes(tree, first, count)
        with pytest.raises(zk.ZkError):
            ctx.merkle_node(0, 2 * m - 1)
    with zk.BatchContext(6, 2, 2) as bc:
        bc.gen_fibsq([1] * 4, [TRACE_A + p for p in range(4)])
        bc.prove_raw()
        heap = 2 * (1 << 8) * 4 - 1
        assert bc.merkle_nodes(0).shape == (heap, 32)
        for tree, first, count in ((0, heap, 1), (0, 1, heap), (9, 0, 1)):
            with pytest.raises(zk.ZkError):
                bc.merkle_nodes(tree, first, count)


# ---- batch trees ------------------------------------------------------------------------------------------------------------
def proof_subtree(batch_nodes, log_batch, p, log_m):
    """Proof p's tree inside a batch heap: the subtree under node 2^log_batch - 1 + p, in heap order."""
    rows = [batch_nodes[(1 << (log_batch + d)) - 1 + (p << d):(1 << (log_batch + d)) - 1 + ((p + 1) << d)] for d in range(log_m + 1)]
    return np.concatenate(rows)


@pytest.mark.parametrize("hash_name,log_n,log_b,log_batch", [
    ("sha256", 6, 2, 0), ("sha256", 6, 2, 2), ("sha256", 8, 3, 4), ("sha256", 11, 3, 2),
    ("field", 5, 2, 0), ("field", 6, 2, 2), ("field", 8, 3, 4), ("field", 11, 3, 2),
])
def test_batch_trees_every_node_after_a_second_batch(zk, orc, heaps, hash_name, log_n, log_b, log_batch):
    """Every node of every proof's tree in the batch heaps (fused composition / fold leaves, the host-built levels that
    scatter_kernel copies back) after a batch of other seeds on the same batch context."""
    h = HASH_OF[hash_name]
    batch = 1 << log_batch
    with zk.BatchContext(log_n, log_b, log_batch, hash=hash_name) as bc:
        for base in (TRACE_A, TRACE_B):
            a1s = [base + 977 * p for p in range(batch)]
            bc.gen_fibsq([1] * batch, a1s)
            bc.prove_raw()
        trees = [bc.merkle_nodes(tr) for tr in range(log_n + 2)]
    orc.set_hash(h)
    try:
        refs = [orc.prove(log_n, log_b, 1, a1s[p], want_vectors=True) for p in range(batch)]
    finally:
        orc.set_hash(orc.HASH_SHA256)
    for p, ref in enumerate(refs):
        assert ref.rc == 0
        for tr, layer in enumerate([ref.f_eval] + ref.cp_layers):
            log_m = len(layer).bit_length() - 1
            assert_nodes(proof_subtree(trees[tr], log_batch, p, log_m), heaps.build(h, layer),
                         f"{hash_name} batch 2^{log_batch} ({log_n}, {log_b}) proof {p} tree {tr}")
