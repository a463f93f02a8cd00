"""A covering walk through the settings of one live batch and its verifier (tests/test_batch_walk.py, tests/test_gpu_batch_walk.py;
DESIGN.md 7d "Reconfiguring a live context").  The shape of tests/settings_walk.py, for zk_batch / zk_verifier.

A zk_batch keeps state from one zk_batch_prove to the next: the gather buffers (re-sized by zk_batch_set_queries and, by another route,
by the format setters), d_work (allocated by the first format other than (K, coset, D) = (1, off, 0) and kept), the tables of the
final polynomials (swapped when D changes), the Grinder (created by the first zk_batch_set_grinding above 10 bits), the mailbox
sequence and the staging buffer of the host-built tree levels, skipped_trees / tree_steps / proved_fold / proved_stop behind
zk_batch_merkle_nodes, the thread pool, the trace state, and the fused launch chain that only (1, off, 0) takes.  Merkle caps, shared
proofs and row leaves add tree_cap[], the pinned buffer h_cap / d_cap / cap_words of a cap deeper than the mailbox holds (bset_format
allocates and gives it back, digest_level_post_kernel fills it), proved and rows_tree0, skipped_trees = ~1 after a shared proof, proof
0's share of every layer, tree and challenge entry overwritten from id 1 on by the one FRI of a shared proof, and an f stage that runs
at the batch's width or at width one with the mailbox sequence running on across both.  A wrong proof after a setter call shows only
on a batch that has proved before in another configuration.  walk(log_n, log_b, shares) is a tuple of Steps -- one value for every
factor of values() -- that starts at the configuration of a fresh batch and is extended greedily, one step at a time, by the candidate
(drawn from a fixed seed) that meets most of the conditions still open:

  * every pair of values of two different factors occurs in some step                                     (missing_pairs)
  * every ordered change of one factor from one value to another occurs between two consecutive steps     (missing_changes)
  * the formats (1, off, 0) -- the fused launch chain -- and (3, on, largest D) each occur three times, isolated   (settings_walk.isolated)
  * of the isolated (1, off, 0) steps with SHA-256, two have host levels on and two have them off         (host_split)
  * step 0 is the fresh batch: (1, off, 0), q = 1, no grinding, SHA-256, no cap, zk_batch_prove           (fresh_start)
  * some step holds q = 16, K = 3, one-value leaves and a last group shorter than K                       (largest_decommitment)
  * ... and some such step is a shared proof without row leaves and without a cap: the most openings the gather buffers hold for
    a shared proof                                                                                        (largest_shared_decommitment)
  * a zk_batch_prove in the fused format (1, off, 0) directly after a shared proof, twice, once after row leaves; a shared proof in
    (1, off, 0) directly after a zk_batch_prove of another format: the fused chain of the shared FRI and the batch's share proof 0's
    layers and d_chal[0]                                                                                  (call_isolated)
  * the verifier's shared setting -- plain, shared, shared with rows -- makes all six ordered changes between consecutive steps, one
    of them together with a change of the cap                                                             (verifier_shared_changes)
  * among the SHA-256 steps whose f stage runs at the batch's width: cap 0, a cap below the host's share of a tree and a cap at or
    above it (the host hashes nothing), each with host levels on and with them off                        (cap_vs_host_share)
  * cap 8 in a zk_batch_prove and in a shared proof without rows, and a shared proof with rows and cap 8 directly between two such
    steps; with log_batch + min(8, L - 1) > 10 the former post their f cap through digest_level_post_kernel into the pinned buffer
    and the latter's f stage, one tree wide, goes through the mailbox (8 -> 0 or 4 -> 8 is among the changes)   (deep_cap)
  * six steps of index >= 1 fit a failed proof before the good one: (1, off, 0); D > 0; K = 3 with coset leaves and D = 0; a shared
    proof; a shared proof with rows; a zk_batch_prove with a cap                                          (fault_steps)
  * two consecutive pairs of steps differ in nothing that the proof bytes depend on                       (twins)
  * two consecutive zk_batch_prove steps differ in `rows` and in nothing the bytes depend on              (rows_twins)
  * at most MAX_STEPS steps

A batch of one refuses zk_batch_prove_shared: with shares = False, `call` has the single value "each", `rows` is still toggled, and the
conditions that need a shared proof are not asked for.  The conditions are checked here once (assert in walk) and one by one in
tests/test_batch_walk.py.  expected() is the reference of a step: cap_ref.proof per proof of a zk_batch_prove (with cap 0 the bytes of
stop_ref.stop_proof), shared_ref.proof or rows_ref.proof for the one proof of a zk_batch_prove_shared, with the commit phases looked up
in settings_walk's unbounded table."""
import collections
import contextlib
import functools
import itertools
import random

import cap_ref
import fold_ref
import rows_ref
import settings_walk as sw
import shared_ref
import stop_ref

MAX_STEPS = 32
SEED = 20261018
MAX_QUERIES = 16                                            # zk_batch_set_queries' limit
ENTRIES = ("gen_fibsq", "set_traces")
SEED_SETS = {"A": 3141592, "B": 271828}                     # proof p proves fibsq(1, base + p)
FACTORS = ("hash", "q", "bits", "K", "coset", "D", "host", "threads", "entry", "seeds", "cap", "call", "rows")
INVISIBLE = ("host", "threads", "entry")                    # must not change a byte; `rows` neither, in a zk_batch_prove (visible())
Step = collections.namedtuple("Step", FACTORS, defaults=(0, "each", False))
# What zk_batch_create leaves behind: the test calls no setter before step 0.  (Host levels are on where the CPU has SHA extensions and
# the pool has min(hardware threads, 16) threads; both are invisible, so a machine where they differ proves the same bytes.)
FRESH = Step(hash=0, q=1, bits=0, K=1, coset=False, D=0, host=1, threads=16, entry="gen_fibsq", seeds="A", cap=0, call="each", rows=False)
PLAIN = (1, False, 0)
MAX_HOST_LOG = 10                                           # the mailbox holds 2^10 digests (kMaxHostLog)


def values(log_n, log_b, shares=True):
    """factor -> its values for a batch of this shape; shares: the batch holds more than one proof (log_batch >= 1)."""
    return {"hash": (0, 1), "q": (1, 3, MAX_QUERIES), "bits": (0, 6, 12), "K": (1, 2, 3), "coset": (False, True),
            "D": (0, 2, sw.largest_stop(log_n, log_b)), "host": (0, 1), "threads": (1, 4, 16), "entry": ENTRIES, "seeds": ("A", "B"),
            "cap": (0, 4, 8), "call": ("each", "shared") if shares else ("each",), "rows": (False, True)}


def big_format(log_n, log_b):
    return (3, True, sw.largest_stop(log_n, log_b))


def seeds_of(step, batch):
    """(a0s, a1s) of the batch's traces in this step."""
    return [1] * batch, [SEED_SETS[step.seeds] + p for p in range(batch)]


def tree_steps(log_n, step):
    """{tree id: log2 of the values per leaf} of the trees a proof of this step's format builds (every other id of 0 .. log_n + 1 is not
    built): f and the last layer keep one-value leaves, the tree over a group's input has that group's cosets as leaves, and the layer a
    stopped proof ends at gets no tree."""
    grp = fold_ref.groups(log_n - step.D, step.K)
    out = {0: 0, 1: grp[0][1] if step.coset else 0}
    for j, (r0, s) in enumerate(grp):
        if j + 1 < len(grp):
            out[1 + r0 + s] = grp[j + 1][1] if step.coset else 0
        elif step.D == 0:
            out[1 + r0 + s] = 0
    return out


def visible(step):
    """What the bytes of the step's proof(s) depend on: every factor but the invisible ones, and `rows` only in a shared proof."""
    return tuple(getattr(step, f) for f in FACTORS if f not in INVISIBLE and f != "rows") + (step.rows and step.call == "shared",)


def shared_kind(step):
    """The verifier's shared setting as a name: "plain" = (0, False), "shared" = (log_batch, False), "rows" = (log_batch, True)."""
    return "plain" if step.call == "each" else "rows" if step.rows else "shared"


def verifier_shared(step, log_batch):
    """The (log_batch, rows) of zk_verifier_set_shared in this step."""
    return (log_batch, step.rows) if step.call == "shared" else (0, False)


def host_share(log_n, log_b, log_batch):
    """Levels of a proof's f tree that the host threads hash with SHA-256 and host levels on, by the rule of DESIGN.md 7f (`bextra`): as
    many as the mailbox of 2^10 digests holds for the whole batch, at most 8, at most L - 1, and none where that leaves fewer than 3.  A
    batch of one is the one-call prover with its top 8 levels on the host."""
    L = log_n + log_b
    h = min(MAX_HOST_LOG - log_batch, 8, L - 1) if log_batch else min(8, L - 1)
    return h if h >= 3 else 0


def pinned_cap_words(log_n, log_b, log_batch, cap):
    """Words of the pinned buffer a batch holds for a cap deeper than the mailbox (include/zkstark_amd.h, zk_batch_set_merkle_cap): 0
    unless cap > 0 and the f cap of the whole batch, 2^(log_batch + ce_f) digests with ce_f = min(cap, L - 1), is more than 2^10."""
    e = log_batch + min(cap, log_n + log_b - 1)
    return 16 + (8 << e) if log_batch and cap and e > MAX_HOST_LOG else 0


# ---- the conditions, each on its own --------------------------------------------------------------------------------------------
def all_pairs(vals):
    return {((f, a), (g, b)) for f, g in itertools.combinations(FACTORS, 2) for a in vals[f] for b in vals[g]}


_PAIRS = tuple((i, f, j, g) for (i, f), (j, g) in itertools.combinations(enumerate(FACTORS), 2))


def pairs_of(step):
    return {((f, step[i]), (g, step[j])) for i, f, j, g in _PAIRS}


def all_changes(vals):
    return {(f, a, b) for f in FACTORS for a in vals[f] for b in vals[f] if a != b}


def changes_of(prev, step):
    return {(f, a, b) for f, a, b in zip(FACTORS, prev, step) if a != b}


def missing_pairs(steps, vals):
    return all_pairs(vals) - set().union(*(pairs_of(s) for s in steps))


def missing_changes(steps, vals):
    return all_changes(vals) - set().union(*(changes_of(a, b) for a, b in zip(steps, steps[1:])))


def host_split(steps):
    """{host: indices} of the isolated (1, off, 0) steps with SHA-256: with host levels on, the host threads write the staging buffer
    and the last launches scatter it; with them off, every level is the device's."""
    at = [i for i in sw.isolated(steps, PLAIN) if steps[i].hash == 0]
    return {h: [i for i in at if steps[i].host == h] for h in (0, 1)}


def fresh_start(steps):
    return all(getattr(steps[0], f) == getattr(FRESH, f) for f in FACTORS if f not in INVISIBLE)


def largest_decommitment(steps, log_n):
    return [i for i, s in enumerate(steps) if s.q == MAX_QUERIES and s.K == 3 and not s.coset and sw.short_last_group(log_n, s)]


def largest_shared_decommitment(steps, log_n):
    """The most openings the gather buffers must hold for a shared proof: 3M f tuples with whole paths and the widest group tuples."""
    return [i for i in largest_decommitment(steps, log_n) if steps[i].call == "shared" and not steps[i].rows and steps[i].cap == 0]


def call_isolated(steps):
    """{name: indices i}: "each_after_shared" a zk_batch_prove in (1, off, 0) directly after a shared proof, "each_after_rows" those of
    them that follow row leaves, "shared_after_each" a shared proof in (1, off, 0) directly after a zk_batch_prove of another format."""
    after = [i for i in range(1, len(steps)) if steps[i].call == "each" and sw.fmt(steps[i]) == PLAIN and steps[i - 1].call == "shared"]
    return {"each_after_shared": after, "each_after_rows": [i for i in after if steps[i - 1].rows],
            "shared_after_each": [i for i in range(1, len(steps)) if steps[i].call == "shared" and sw.fmt(steps[i]) == PLAIN
                                  and steps[i - 1].call == "each" and sw.fmt(steps[i - 1]) != PLAIN]}


def call_isolated_goals(steps):
    at = call_isolated(steps)
    return min(len(at["each_after_shared"]), 2) + bool(at["each_after_rows"]) + bool(at["shared_after_each"]), 4


SHARED_KINDS = ("plain", "shared", "rows")


def verifier_shared_changes(steps):
    """{(from, to): indices i} of the ordered changes of the verifier's shared setting between steps i - 1 and i, and under "with_cap"
    those of them where the cap changes in the same step."""
    out = {(a, b): [] for a in SHARED_KINDS for b in SHARED_KINDS if a != b}
    out["with_cap"] = []
    for i in range(1, len(steps)):
        a, b = shared_kind(steps[i - 1]), shared_kind(steps[i])
        if a != b:
            out[(a, b)].append(i)
            if steps[i - 1].cap != steps[i].cap:
                out["with_cap"].append(i)
    return out


def verifier_shared_goals(steps):
    return sum(bool(v) for v in verifier_shared_changes(steps).values()), 7


def cap_vs_host_share(steps, log_n, log_b, log_batch):
    """{host: {"none" | "below" | "at": indices}} of the SHA-256 steps whose f stage runs at the batch's width (every step but a shared
    proof with rows), by where the f tree's cap lies against the host's share: no cap, a cap below the share (the host hashes from its
    share down to the cap), a cap at or above it (the host hashes nothing)."""
    h, L = host_share(log_n, log_b, log_batch), log_n + log_b
    out = {host: {"none": [], "below": [], "at": []} for host in (0, 1)}
    for i, s in enumerate(steps):
        if s.hash == 0 and shared_kind(s) != "rows":
            ce = cap_ref.c_eff(s.cap, L)
            out[s.host]["none" if ce == 0 else "below" if ce < h else "at"].append(i)
    return out


def cap_vs_host_share_goals(steps, log_n, log_b, log_batch):
    return sum(bool(v) for cells in cap_vs_host_share(steps, log_n, log_b, log_batch).values() for v in cells.values()), 6


def share_batches(shares):
    """The batch sizes cap_vs_host_share is asked for: what tests/test_gpu_batch_walk.py walks, 2^1 .. 2^3 proofs, or one."""
    return (1, 2, 3) if shares else (0,)


def deep_cap(steps, shares=True):
    """{"each": the zk_batch_prove steps with cap 8, "shared": the shared proofs without rows with cap 8, "rows_between": the shared
    proofs with rows and cap 8 whose two neighbours are both among the former, "leave" / "enter": the steps that go from cap 8 to a
    smaller one / back to 8}."""
    deep = [i for i, s in enumerate(steps) if s.cap == 8 and shared_kind(s) != "rows"]
    out = {"each": [i for i in deep if steps[i].call == "each"],
           "leave": [i for i in range(1, len(steps)) if steps[i - 1].cap == 8 and steps[i].cap < 8],
           "enter": [i for i in range(1, len(steps)) if steps[i - 1].cap < 8 and steps[i].cap == 8]}
    if shares:
        out["shared"] = [i for i in deep if steps[i].call == "shared"]
        out["rows_between"] = [i for i, s in enumerate(steps) if s.cap == 8 and shared_kind(s) == "rows" and i - 1 in deep and i + 1 in deep]
    return out


def deep_cap_goals(steps, shares=True):
    at = deep_cap(steps, shares)
    return sum(bool(v) for v in at.values()), len(at)


def twins(steps):
    """Indices i where steps i and i + 1 differ, but in nothing the bytes depend on."""
    return [i for i, (a, b) in enumerate(zip(steps, steps[1:]))
            if a != b and all(getattr(a, f) == getattr(b, f) for f in FACTORS if f not in INVISIBLE)]


def rows_twins(steps):
    """Indices i where steps i and i + 1 are both a zk_batch_prove and differ in `rows` (zk_batch_set_shared_rows is called between
    them) and otherwise at most in invisible factors: the same bytes again."""
    return [i for i, (a, b) in enumerate(zip(steps, steps[1:])) if a.rows != b.rows and a.call == b.call == "each" and visible(a) == visible(b)]


FAULT_KINDS = ("plain", "stopped", "coset_k3")
MORE_FAULT_KINDS = ("shared", "shared_rows", "capped")


def fault_kinds(shares=True):
    return FAULT_KINDS + (MORE_FAULT_KINDS if shares else ("capped",))


def _fits(kind, s):
    if kind == "plain":
        return sw.fmt(s) == PLAIN
    if kind == "stopped":
        return s.D > 0
    if kind == "shared":
        return s.call == "shared" and not s.rows
    if kind == "shared_rows":
        return s.call == "shared" and s.rows
    if kind == "capped":
        return s.call == "each" and s.cap > 0
    return s.K == 3 and s.coset and s.D == 0


def fault_steps(steps, kinds=FAULT_KINDS):
    """{index: kind} of the steps that prove corrupted traces first: the earliest step of index >= 1 that fits each kind (step 0 is left
    alone, so that every failed proof happens on a batch that has proved before).  The three kinds of the format come first, so
    fault_steps(steps) is part of fault_steps(steps, fault_kinds(shares)): a kind without a fitting step is left out."""
    out = {}
    for kind in kinds:
        for i, s in enumerate(steps):
            if i >= 1 and _fits(kind, s) and i not in out:
                out[i] = kind
                break
    return out


def fault_message(step):
    """What zk_batch_prove and zk_batch_prove_shared say about a trace that breaks the constraints (ZK_ERR_CHECK; csrc/batch.hip,
    prover.rs:238)."""
    return f"final FRI layer has degree >= 2^{step.D}" if step.D else "last FRI layer is not constant"


def fault_culprit(step, broken):
    """Whom the message blames: zk_batch_prove the lowest broken proof, zk_batch_prove_shared cannot tell."""
    return "some trace of the batch" if step.call == "shared" else f"proof {min(broken)} of the batch"


def broken_proofs(steps, i, log_batch):
    """The proofs whose trace is corrupted before fault step i: proof 1 alone; on the second fault step of the three format kinds two
    proofs, of which the lower one is reported; a batch of one has only proof 0."""
    if log_batch == 0:
        return (0,)
    first = sorted(fault_steps(steps))
    if i in first and first.index(i) == 1:
        return (1, 3) if log_batch >= 2 else (0, 1)
    return (1,)


def unmet(steps, log_n, log_b, shares=True):
    """Names of the conditions `steps` does not meet."""
    vals = values(log_n, log_b, shares)
    out = []
    if missing_pairs(steps, vals):
        out.append("pairs")
    if missing_changes(steps, vals):
        out.append("changes")
    for triple in (PLAIN, big_format(log_n, log_b)):
        if len(sw.isolated(steps, triple)) < 3:
            out.append(f"format {triple}")
    if min(len(v) for v in host_split(steps).values()) < 2:
        out.append("host split")
    if not fresh_start(steps):
        out.append("fresh start")
    if not largest_decommitment(steps, log_n):
        out.append("largest decommitment")
    if shares and not largest_shared_decommitment(steps, log_n):
        out.append("largest shared decommitment")
    if shares and call_isolated_goals(steps)[0] < 4:
        out.append("call isolated")
    if shares and verifier_shared_goals(steps)[0] < 7:
        out.append("verifier shared changes")
    if any(cap_vs_host_share_goals(steps, log_n, log_b, lb)[0] < 6 for lb in share_batches(shares)):
        out.append("cap vs host share")
    if len(set(deep_cap_goals(steps, shares))) > 1:
        out.append("deep cap")
    if sorted(fault_steps(steps, fault_kinds(shares)).values()) != sorted(fault_kinds(shares)):
        out.append("fault steps")
    if len(twins(steps)) < 2:
        out.append("twins")
    if not rows_twins(steps):
        out.append("rows twins")
    if len(steps) > MAX_STEPS:
        out.append("length")
    return out


# ---- the generator --------------------------------------------------------------------------------------------------------------
def _random_step(rng, vals, prev):
    s = Step(*(rng.choice(vals[f]) for f in FACTORS))
    if rng.random() < 0.75:                                  # the traces mostly alternate: a stale layer is then a wrong layer
        s = s._replace(seeds=[a for a in vals["seeds"] if a != prev.seeds][0])
    return s


def _mutated(rng, vals, prev, factors, count):
    s = prev
    for f in rng.sample(factors, count):
        s = s._replace(**{f: rng.choice(vals[f])})
    return s


def _met(steps, log_n, log_b, shares):
    """What the conditions on caps, shared proofs and rows have found in `steps` so far, as one dict of index lists."""
    out = {("cell", host, name): at for host, cells in cap_vs_host_share(steps, log_n, log_b, share_batches(shares)[0]).items()
           for name, at in cells.items()}
    out.update({("deep", k): at for k, at in deep_cap(steps, shares).items()})
    out["rows twins"] = rows_twins(steps)
    if shares:
        out.update({("call", k): at for k, at in call_isolated(steps).items()})
        out[("call", "each_after_shared")] = out[("call", "each_after_shared")][1:]    # open until the second one
        out.update({("verifier", k): at for k, at in verifier_shared_changes(steps).items()})
        out["largest shared"] = largest_shared_decommitment(steps, log_n)
    return out


def _gain(met, tail, log_n, log_b, shares):
    """How many of the sub-goals still open in `met` the last step of `tail` (the last two steps and a candidate) closes: whatever the
    condition functions find in the tail alone that they had not found in the steps."""
    found = _met(tail, log_n, log_b, shares)
    if shares:
        found[("call", "each_after_shared")] = call_isolated(tail)["each_after_shared"]
    return sum(bool(found[k]) and not met[k] for k in met)


@functools.lru_cache(maxsize=None)
def walk(log_n, log_b, shares=True, seed=SEED):
    """The walk for a batch of shape (log_n, log_b), as a tuple of Steps; among the batches that can share (shares: log_batch >= 1) and
    among those that cannot, the batch size changes no step."""
    rng = random.Random(f"batch/{seed}/{log_n}/{log_b}/{int(shares)}")
    vals = values(log_n, log_b, shares)
    formats = (PLAIN, big_format(log_n, log_b))
    kinds = fault_kinds(shares)
    steps = [FRESH]
    pairs, changes = missing_pairs(steps, vals), missing_changes(steps, vals)
    while unmet(steps, log_n, log_b, shares) and len(steps) < MAX_STEPS:
        prev = steps[-1]
        cands = [_random_step(rng, vals, prev) for _ in range(600)]
        cands += [_mutated(rng, vals, prev, FACTORS, rng.randint(1, 5)) for _ in range(200)]
        cands += [_mutated(rng, vals, prev, INVISIBLE + ("rows",), rng.randint(1, 4)) for _ in range(50)]
        need_fault = set(kinds) - set(fault_steps(steps, kinds).values())
        split = host_split(steps)
        met = _met(steps, log_n, log_b, shares)
        few_isolated = {triple: len(sw.isolated(steps, triple)) < 3 for triple in formats}
        need_largest, need_twins = not largest_decommitment(steps, log_n), len(twins(steps)) < 2
        deep = deep_cap(steps, shares)
        prev_deep = prev.cap == 8 and shared_kind(prev) != "rows"
        best, best_score = None, None
        for c in cands:
            score = len(pairs_of(c) & pairs) + 3 * len(changes_of(prev, c) & changes)
            for triple in formats:
                if sw.fmt(c) == triple:
                    if sw.fmt(prev) == triple:
                        score -= 100                         # would spoil an isolated occurrence
                    elif few_isolated[triple]:
                        score += 40
            if sw.fmt(c) == PLAIN != sw.fmt(prev) and c.hash == 0 and len(split[c.host]) < 2:
                score += 30
            if need_largest and largest_decommitment([c], log_n):
                score += 40
            score += 40 * sum(_fits(k, c) for k in need_fault)
            if need_twins and twins([prev, c]):
                score += 25
            score += 40 * _gain(met, steps[-2:] + [c], log_n, log_b, shares)
            if shares and not deep["rows_between"]:          # the two steps before the one that closes it
                if c.cap == 8 and shared_kind(c) == "rows" and prev_deep:
                    score += 30
                elif c.cap == 8 and shared_kind(c) != "rows" and not prev_deep:
                    score += 10
            if best_score is None or score > best_score:
                best, best_score = c, score
        steps.append(best)
        pairs -= pairs_of(best)
        changes -= changes_of(prev, best)
    left = unmet(steps, log_n, log_b, shares)
    assert not left, (left, len(steps))
    return tuple(steps)


# ---- the reference proofs -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _unbounded_commit_cache():
    """settings_walk's unbounded table of commit phases, with the two models of shared proofs looked up in it as well."""
    mods = (shared_ref, rows_ref)
    saved = [m.committed for m in mods]
    with sw._unbounded_commit_cache():
        for m in mods:
            m.committed = sw._memoised(m)
        try:
            yield
        finally:
            for m, f in zip(mods, saved):
                m.committed = f


forget_commits = sw.forget_commits


def model_of(step):
    """The module whose proof() and verify() are the reference of this step."""
    return cap_ref if step.call == "each" else rows_ref if step.rows else shared_ref


def expected(orc, shape, step, p=0, log_batch=0):
    """The reference of `step` for `shape` = (log_n, log_b): in a zk_batch_prove step the proof of proof p of the batch (cap_ref.proof), in
    a shared step the ONE proof of the 2^log_batch traces (shared_ref.proof, or rows_ref.proof with row leaves; p is not looked at).  Its
    .data, .state, .public_last (a list in a shared step), .coef and .c (the model's Committed) are read as they are.  Host levels, threads
    and the trace entry point are not arguments: they must not change a byte."""
    log_n, log_b = shape
    with _unbounded_commit_cache():
        if step.call == "each":
            return cap_ref.proof(orc, log_n, log_b, step.q, step.hash, step.K, step.coset, step.D, step.cap, step.bits, SEED_SETS[step.seeds] + p)
        assert log_batch >= 1, "a batch of one makes no shared proof"
        return model_of(step).proof(orc, log_n, log_b, log_batch, step.q, step.hash, step.K, step.coset, step.D, step.cap, step.bits,
                                    SEED_SETS[step.seeds])


def expected_len(shape, step, log_batch=0):
    """The length of the step's proof by the model's own formula."""
    log_n, log_b = shape
    args = (log_n, log_b, step.q, step.bits, step.K, step.coset, step.D, step.cap)
    return cap_ref.proof_len(*args) if step.call == "each" else model_of(step).proof_len(*args, log_batch)


def model_verdict(orc, shape, step, data, state, public_last, log_batch=0):
    """The check number of the step's plain-Python verifier for `data` (0 = accepted); state None: not strict."""
    log_n, log_b = shape
    tail = (step.hash, step.q, step.bits, step.K, step.coset, step.D, step.cap)
    if step.call == "each":
        return cap_ref.verify(orc, data, state, log_n, log_b, public_last, *tail)
    return model_of(step).verify(orc, data, state, log_n, log_b, list(public_last), log_batch, *tail)


def bit_flips(shape, i, batch, plen):
    """Step i's three mutations of one of its proofs, [(proof, byte, bit)], drawn from the step's own seeded Random: one in the first
    64 bytes (the first root, the alphas, the second root), one in the middle third, one inside the last 32 bytes (the last digest of
    the last opened path)."""
    rng = random.Random(f"batch flips/{SEED}/{shape[0]}/{shape[1]}/{i}")
    spans = ((0, 64), (plen // 3, 2 * plen // 3), (plen - 32, plen))
    return [(rng.randrange(batch), rng.randrange(lo, hi), rng.randrange(8)) for lo, hi in spans]
