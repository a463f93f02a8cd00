"""Helpers of tests/test_gpu_handover_soak.py: the grid, the planner mirror of a whole proof, the proof layout, the load generator.

The soak runs every case on the SAME buffers with two inputs in turn (A, B, A, B, ...), so that every address a hand-over reads
holds the other input's value until the producer's store arrives: a consumer that reads too early gets bytes that are wrong
for this run, and every run is compared with the CPU oracle's result for its input (never with the library's own first run).
tests/test_handover_soak_grid.py checks on the CPU, from the planner mirror (tests/merkle_plans.py), that the rows below reach
the hand-overs they were chosen for.
"""
import random
import threading
import time

import merkle_plans as mp
import verify_corpus

SEED_A, SEED_B = verify_corpus.SEEDS                      # a1 of the two traces every case alternates (a0 = 1); A is 3141592
HASH_NAMES = {mp.SHA: "sha256", mp.FIELD: "field"}
DEFAULT_HOST_LEVELS = (8, 9)                              # zk_ctx_create: host_top, host_tail where the host has SHA extensions
LOADS = ("uniform", "uneven")
LOAD_LOG_N, LOAD_LOG_B = 19, 3                            # the load generator's proofs: domain 2^22
CUS = 256                                                 # a launch of more workgroups than this is not resident at once


# ---- part 2: whole proofs ---------------------------------------------------------------------------------------------------
class Row:
    """One prover setting; `pairs` times (A, B) are proved under each kind of load.  The floors are 50 pairs for domains up to
    2^16 and 30 above; the counts below are what fills about 2 s per case on the MI355X (measured: the test module's docstring)."""

    def __init__(self, log_n, log_b, h, host_levels=None, pairs=0, early=False, q=1, fold_log=1, grind_bits=0, lat=mp.LATENCY_LOG):
        self.lat = lat                      # zk_dev_set_merkle_latency_log while the row runs (process-wide; the default otherwise)
        self.log_n, self.log_b, self.h, self.host_levels, self.early = log_n, log_b, h, host_levels, early
        self.q, self.fold_log, self.grind_bits, self.pairs = q, fold_log, grind_bits, pairs

    @property
    def id(self):
        lv = "default" if self.host_levels is None else "host%d.%d" % self.host_levels
        extra = (f"-q{self.q}" if self.q != 1 else "") + ("-early" if self.early else "") + \
            (f"-fold{self.fold_log}" if self.fold_log != 1 else "") + (f"-grind{self.grind_bits}" if self.grind_bits else "") + \
            (f"-lat{self.lat}" if self.lat != mp.LATENCY_LOG else "")
        return f"{HASH_NAMES[self.h]}-{self.log_n}.{self.log_b}-{lv}{extra}"

    @property
    def floor(self):
        return 50 if self.log_n + self.log_b <= 16 else 30

    @property
    def ref_key(self):
        """What the reference proof depends on (host_levels and early launch change who computes a node and when, not its value)."""
        return (self.log_n, self.log_b, self.h, self.q, self.fold_log, self.grind_bits)

    @property
    def effective_host_levels(self):
        return DEFAULT_HOST_LEVELS if self.host_levels is None else self.host_levels


S, F = mp.SHA, mp.FIELD
PROOF_ROWS = [
    # N = 2^13: one latency launch per tree
    Row(10, 3, S, (0, 0), 600), Row(10, 3, S, None, 1000), Row(10, 3, F, (0, 0), 500), Row(10, 3, F, None, 550),
    # N = 2^16: still below the latency switch
    Row(13, 3, S, (0, 0), 400), Row(13, 3, S, (5, 6), 600), Row(13, 3, S, None, 650),
    Row(13, 3, F, (0, 0), 380), Row(13, 3, F, (5, 6), 380), Row(13, 3, F, None, 380),
    # N = 2^18: a throughput launch, then the latency phase
    Row(15, 3, S, None, 400), Row(15, 3, F, None, 250),
    # N = 2^20, the metric's second size (the field hash's two oracle proofs take 1.5 s: kept).  With the default latency log every
    # merkle_wg_kernel launch of a proof has at most 256 workgroups, one per CU; the last row moves the switch to 2^19 nodes, where
    # the tree of 2^19 leaves is one launch of 512 workgroups with a continuation (as merkle_plans.commit_cases' (19, 19, 0, 0))
    Row(17, 3, S, None, 250), Row(17, 3, S, (0, 0), 240), Row(17, 3, F, None, 160), Row(17, 3, S, (0, 0), 260, lat=19),
    # early launch: the challenge-dependent constant comes through a pinned slot that every second round and every proof reuses
    Row(13, 3, S, None, 550, early=True, q=2), Row(17, 3, S, None, 250, early=True, q=2),
    # folding by 8: every layer on the device, the trees through the stand-alone commitment (no posted values)
    Row(13, 3, S, None, 800, fold_log=3), Row(13, 3, F, None, 700, fold_log=3), Row(17, 3, S, None, 300, fold_log=3),
    # g = 14 > kGrindHostMaxBits: the device grinder and its mailbox run between the last root and the openings
    Row(10, 3, S, None, 800, q=7, grind_bits=14),
]


def proof_trees(log_n, log_b, h, host_levels, fold_log=1):
    """The trees a proof commits on the device, as zk_prove_resident (zkstark.hip) does: [(tree, log_m, top, posts_values)].
    top = top_of(): the hand-over depth of SHA-256 trees.  posts_values = mail_of() sets dump_src: the launch also posts the
    layer's values to the host, which folds on from there (host_fold_commit) -- the rounds after it build no tree on the device."""
    L = log_n + log_b
    host_top, host_tail = host_levels if h == mp.SHA else (0, 0)

    def top_of(lg):
        return 0 if not host_top else host_top if lg > host_top else lg - 1

    out = [(0, L, top_of(L), False)]
    if fold_log > 1:                                       # prove_fold_rounds: do_merkle(id, host, feed_tail = false)
        out.append((1, L, top_of(L), False))
        for r0 in range(0, log_n, fold_log):
            tree = 1 + r0 + min(fold_log, log_n - r0)
            out.append((tree, L - (tree - 1), top_of(L - (tree - 1)), False))
        return out
    tail_log = 0
    for tree in range(1, log_n + 2):
        lg = L - (tree - 1)
        if tail_log and tail_log == lg + 1 and lg <= host_tail:     # fri_round_commit: this round runs on the host thread
            tail_log = lg
            continue
        # mail_of: the layer of 2^(host_tail + 1) values is the one whose launch posts values (m.top != 0: the host hashes at all)
        posts = bool(top_of(lg) and host_tail and lg == host_tail + 1)
        if posts:
            tail_log = lg
        out.append((tree, lg, top_of(lg), posts))
    return out


def proof_launches(row_or_args):
    """[(tree, Launch, top, posts_values)] of one proof: posts_values is set on the launch that reaches the hand-over depth of the
    tree whose values go to the host's FRI tail (the dump_src path of merkle_wg_kernel)."""
    r = row_or_args
    out = []
    for tree, lg, top, posts in proof_trees(r.log_n, r.log_b, r.h, r.effective_host_levels, r.fold_log):
        plan = mp.plan(lg, r.h, counter=True, top=top, lat=r.lat)
        for i, la in enumerate(plan):
            out.append((tree, la, top if top < lg else 0, posts and i == len(plan) - 1))
    return out


def workgroups(la):
    """Workgroups of a merkle_wg_kernel launch: one per 2^j inputs."""
    assert la.kind == "wg"
    return 1 << (la.span - la.k)


def reach(launches):
    """What a list of proof_launches() / commit launches reaches, as a set of names (tests/test_handover_soak_grid.py)."""
    got = set()
    for _, la, top, posts in launches:
        if la.kind != "wg":
            continue
        n = workgroups(la)
        if la.j2 > 0 and n > 1:
            got.add("continuation")
        if la.j2 == 0 and top > 0 and n > 1 and la.depth - la.k == top and not posts:
            got.add("relaxed post")
        if n > CUS:
            got.add("not resident at once")
        if posts:
            assert la.leaf and la.depth - la.k - la.j2 == top and top > 0
            got.add("posts values")
    return got


# ---- the proof's layout: where a differing byte falls ---------------------------------------------------------------------------
def proof_fields(log_n, log_b, q=1, bits=0, K=1):
    """[(name, first byte, end)] of a proof (transcript.hpp: proof_data_len); K = 1 is the reference's layout."""
    L = log_n + log_b
    groups = [(r0, min(K, log_n - r0)) for r0 in range(0, log_n, K)]
    out, pos = [], 0

    def add(name, n):
        nonlocal pos
        out.append((name, pos, pos + n))
        pos += n

    add("root of tree 0 (f)", 32)
    add("alphas", 12)
    add("root of tree 1 (cp)", 32)
    for r0, s in groups:
        add(f"beta of round {r0}", 4)
        add(f"root of tree {1 + r0 + s}", 32)
    add("free term", 4)
    if bits:
        add("nonce", 8)
    add("query raws", 4 * q)
    for k in range(q):
        for j, what in enumerate(("f(x)", "f(gx)", "f(ggx)", "cp(x)")):
            add(f"query {k}: value of the opening {what}", 4)
            add(f"query {k}: path length of the opening {what}", 8)
            for d in range(L):
                add(f"query {k}: opening {what}, path node {d} (tree {0 if j < 3 else 1}, depth {L - d})", 32)
        for r0, s in groups:
            add(f"query {k}: the {1 << s} opened values of layer {1 + r0}", 4 << s)
            for t in range(1 << s):
                add(f"query {k}: layer {1 + r0} opening {t}, path length", 8)
                for d in range(L - r0):
                    add(f"query {k}: layer {1 + r0} opening {t}, path node {d} (tree {1 + r0}, depth {L - r0 - d})", 32)
    return out


def first_difference(got, want):
    n = min(len(got), len(want))
    for i in range(0, n, 4096):
        if got[i:i + 4096] != want[i:i + 4096]:
            return next(j for j in range(i, min(i + 4096, n)) if got[j] != want[j])
    return n if len(got) != len(want) else None


def locate(offset, log_n, log_b, q=1, bits=0, K=1):
    for name, a, b in proof_fields(log_n, log_b, q, bits, K):
        if a <= offset < b:
            return name
    return "past the end of the proof"


def describe_mismatch(what, it, load, got, want, layout):
    """The report of a differing proof: case, iteration, load, first differing byte and the root or opening it falls in."""
    if got.state != want.state and got.data == want.data:
        return f"{what}: iteration {it} under {load} load: the proof bytes agree, the channel state differs"
    off = first_difference(got.data, want.data)
    return (f"{what}: iteration {it} (trace {'AB'[it & 1]}) under {load} load: proof differs from the reference first at byte {off} "
            f"of {len(want.data)} (got {len(got.data)}): {locate(off, *layout)}")


# ---- part 3: every node --------------------------------------------------------------------------------------------------------
LEAF_SEED_B = 7919            # the second leaf set: Heaps.leaves' generator with this added to its seed
COMMIT_PAIRS_FLOOR = 30
# (hash, log_m, lat, top, log_parts, pairs): (log_m, lat, top, log_parts) are rows of merkle_plans.commit_cases
COMMIT_CASES = [
    (S, 13, 17, 3, 0, 1200),    # a continuation, then the last workgroup posts 2^3 digests
    (S, 12, 17, 3, 0, 2500),    # the relaxed post of 2^3 digests from 8 workgroups
    (S, 16, 12, 8, 1, 1000),     # leaves in all-to-all order, a throughput leaf launch, the relaxed post of 2^8 digests
    (S, 17, 17, 8, 0, 650),     # the relaxed post from 256 workgroups of 2^9 leaves
    (S, 19, 19, 0, 0, 125),     # the one-lane SHA-256 form in the continuation, 512 workgroups
    (F, 13, 17, 0, 0, 2400),
    (F, 16, 12, 0, 1, 900),     # interleaved leaves, the field hash's continuation
]


def commit_launches(h, log_m, lat, top):
    """zk_dev_merkle_commit's launches in the shape of proof_launches() (it never posts values)."""
    eff = top if h == mp.SHA and log_m > top else 0
    return [(0, la, eff, False) for la in mp.plan(log_m, h, counter=True, top=eff, lat=lat)]


# ---- part 4: the batch prover ----------------------------------------------------------------------------------------------------
BATCH_ROWS = [(6, 2, 4), (10, 3, 2)]                      # (log_n, log_b, log_batch)
BATCH_PAIRS = {(6, 2, 4): 100, (10, 3, 2): 100}
GRIND_BATCH = (4, 1, 6, 12)                               # log_n, log_b, log_batch, grind_bits: the first chunk is 2^14 nonces
GRIND_FIRST_CHUNK = 1 << 14
GRIND_BATCHES = 20


def batch_a1s(which, batch):
    """The two a1 lists of part 4 (a): list A starts at trace A's seed, list B at a seed far from it."""
    return [(SEED_A, 2718281)[which] + 977 * p for p in range(batch)]


# The two a1 lists of part 4 (b), found by a search with tests/grind_ref.py over a1 = 5000000 + k (tests/test_handover_soak_grid.py
# re-derives the three conditions): "slow" seeds, whose smallest nonce at g = 12 on a (4, 1) proof is >= 2^14, at the indices
# given, and seeds that finish in the first launch everywhere else.
GRIND_SLOW_AT = ((5, 17, 40), (3, 9, 62))
GRIND_LISTS = (
    [5000000, 5000001, 5000002, 5000003, 5000004, 5000153, 5000005, 5000006, 5000007, 5000008, 5000009, 5000010,
     5000011, 5000012, 5000013, 5000014, 5000015, 5000328, 5000016, 5000017, 5000018, 5000019, 5000020, 5000021,
     5000022, 5000023, 5000024, 5000025, 5000026, 5000027, 5000028, 5000029, 5000030, 5000031, 5000032, 5000033,
     5000034, 5000035, 5000036, 5000037, 5000371, 5000038, 5000039, 5000040, 5000041, 5000042, 5000043, 5000044,
     5000045, 5000046, 5000047, 5000048, 5000049, 5000050, 5000051, 5000052, 5000053, 5000054, 5000055, 5000056,
     5000057, 5000058, 5000059, 5000060],
    [5000061, 5000062, 5000063, 5000375, 5000064, 5000065, 5000066, 5000067, 5000068, 5000412, 5000069, 5000070,
     5000071, 5000072, 5000073, 5000074, 5000075, 5000076, 5000077, 5000078, 5000079, 5000080, 5000081, 5000082,
     5000083, 5000084, 5000085, 5000086, 5000087, 5000088, 5000089, 5000090, 5000091, 5000092, 5000093, 5000094,
     5000095, 5000096, 5000097, 5000098, 5000099, 5000100, 5000101, 5000102, 5000103, 5000104, 5000105, 5000106,
     5000107, 5000108, 5000109, 5000110, 5000111, 5000112, 5000113, 5000114, 5000115, 5000116, 5000117, 5000118,
     5000119, 5000120, 5000530, 5000121],
)


def grind_conditions(nonces):
    """The three conditions of a list's smallest nonces: at least two proofs miss the first chunk, none of them proof 0; no two of
    them are neighbours; a proof behind the first of them finishes in the first launch (the compaction then moves a job)."""
    slow = [p for p, w in enumerate(nonces) if w >= GRIND_FIRST_CHUNK]
    return (len(slow) >= 2 and 0 not in slow,
            all(b - a > 1 for a, b in zip(slow, slow[1:])),
            bool(slow) and any(p > slow[0] and w < GRIND_FIRST_CHUNK for p, w in enumerate(nonces)))


# ---- the load generator -----------------------------------------------------------------------------------------------------
class Load:
    """Host threads that keep the GPU busy with real proofs while a case runs: one context (and so one stream) per thread,
    SHA-256 on one and the field hash on the other, back-to-back proofs of a resident 2^22-point trace.  Every proof is compared
    with the thread's first one (which the CPU verifier accepted); a difference or an error is recorded, raises `failed`, and
    stops every thread.  Everything stays in this process.

        load = Load(zk)                  # once: the contexts and the first proofs
        with load.running("uneven"):     # threads start; on exit they are stopped and joined
            ... the case; poll load.failed and leave the loop on the first mismatch anywhere ...
        assert not load.errors           # after the join
        load.close()
    """
    MAX_THREADS = 3

    def __init__(self, zk, hashes=("sha256", "field")):
        assert len(hashes) <= self.MAX_THREADS
        self.zk, self.ctxs, self.first = zk, [], []
        self.failed, self._stop, self.threads, self.errors, self.proofs = threading.Event(), threading.Event(), [], [], 0
        trace = zk.trace_fibsq((1 << LOAD_LOG_N) - 1)
        try:
            for name in hashes:
                ctx = zk.Context(LOAD_LOG_N, LOAD_LOG_B, hash=name)
                self.ctxs.append(ctx)
                ctx.trace_upload(trace)
                p = ctx.prove()
                p.verify(strict=True)
                self.first.append(p)
        except BaseException:
            self.close()
            raise

    def _work(self, i, uneven, seed):
        ctx, first, rng, n = self.ctxs[i], self.first[i], random.Random(seed), 0
        try:
            while not self._stop.is_set():
                p = ctx.prove()
                n += 1
                if p.data != first.data or p.state != first.state:
                    off = first_difference(p.data, first.data)
                    self.errors.append(f"load thread {i} ({ctx.hash}): proof {n} differs from the thread's first proof at byte {off}: "
                                       + locate(off if off is not None else 0, LOAD_LOG_N, LOAD_LOG_B))
                    break
                if uneven:
                    time.sleep(rng.uniform(0.0, 0.002))        # the chip goes from full to empty while the case runs
        except Exception as e:                                 # a ZkError of the library: reported like a mismatch
            self.errors.append(f"load thread {i} ({ctx.hash}): {e!r}")
        if self.errors:
            self.failed.set()
            self._stop.set()
        self.proofs += n

    def start(self, kind, seed=1):
        assert kind in LOADS and not self.threads
        self.errors = []
        self.failed.clear()
        self._stop.clear()
        self.threads = [threading.Thread(target=self._work, args=(i, kind == "uneven", 1000 * seed + i), daemon=True) for i in range(len(self.ctxs))]
        for t in self.threads:
            t.start()

    def stop(self):
        """Stops and joins every thread; returns the failures recorded so far."""
        self._stop.set()
        for t in self.threads:
            t.join()
        self.threads = []
        return list(self.errors)

    def running(self, kind, seed=1):
        return _Running(self, kind, seed)

    def close(self):
        self.stop()
        for c in self.ctxs:
            c.close()
        self.ctxs = []


class _Running:
    def __init__(self, load, kind, seed):
        self.load, self.kind, self.seed = load, kind, seed

    def __enter__(self):
        self.load.start(self.kind, self.seed)
        return self.load

    def __exit__(self, exc_type, exc, tb):
        self.load.stop()                                       # every thread is joined before any assertion is raised
        return False
