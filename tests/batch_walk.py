"""A covering walk through the settings of one live batch and its verifier (tests/test_batch_walk.py, tests/test_gpu_batch_walk.py;
DESIGN.md 7d "Reconfiguring a live context").  The shape of tests/settings_walk.py, for zk_batch / zk_verifier.

A zk_batch keeps state from one zk_batch_prove to the next: the gather buffers (re-sized by zk_batch_set_queries and, by another route,
by the three format setters), d_work (allocated by the first format other than (K, coset, D) = (1, off, 0) and kept), the tables of the
final polynomials (swapped when D changes), the Grinder (created by the first zk_batch_set_grinding above 10 bits), the mailbox
sequence and the staging buffer of the host-built tree levels, skipped_trees / tree_steps / proved_fold / proved_stop behind
zk_batch_merkle_nodes, the thread pool, the trace state, and the fused launch chain that only (1, off, 0) takes.  A wrong proof after a
setter call shows only on a batch that has proved before in another configuration.  walk(log_n, log_b) is a tuple of Steps -- one value
for every factor of values() -- that starts at the configuration of a fresh batch and is extended greedily, one step at a time, by the
candidate (drawn from a fixed seed) that meets most of the conditions still open:

  * every pair of values of two different factors occurs in some step                                     (missing_pairs)
  * every ordered change of one factor from one value to another occurs between two consecutive steps     (missing_changes)
  * the formats (1, off, 0) -- the fused launch chain -- and (3, on, largest D) each occur three times, isolated   (settings_walk.isolated)
  * of the isolated (1, off, 0) steps with SHA-256, two have host levels on and two have them off         (host_split)
  * step 0 is the fresh batch: (1, off, 0), q = 1, no grinding, SHA-256                                   (fresh_start)
  * some step holds q = 16, K = 3, one-value leaves and a last group shorter than K                       (largest_decommitment)
  * three steps of index >= 1 fit a failed proof before the good one: (1, off, 0); D > 0; K = 3 with coset leaves and D = 0  (fault_steps)
  * two consecutive pairs of steps differ in nothing that the proof bytes depend on                       (twins)
  * at most MAX_STEPS steps

The conditions are checked here once (assert in walk) and one by one in tests/test_batch_walk.py.  expected() is the reference proof of
proof p of a step, from stop_ref.stop_proof, with the commit phases looked up in settings_walk's unbounded table."""
import collections
import functools
import itertools
import random

import fold_ref
import settings_walk as sw
import stop_ref

MAX_STEPS = 32
SEED = 20261018
MAX_QUERIES = 16                                            # zk_batch_set_queries' limit
ENTRIES = ("gen_fibsq", "set_traces")
SEED_SETS = {"A": 3141592, "B": 271828}                     # proof p proves fibsq(1, base + p)
FACTORS = ("hash", "q", "bits", "K", "coset", "D", "host", "threads", "entry", "seeds")
INVISIBLE = ("host", "threads", "entry")                    # must not change a byte
Step = collections.namedtuple("Step", FACTORS)
# What zk_batch_create leaves behind: the test calls no setter before step 0.  (Host levels are on where the CPU has SHA extensions and
# the pool has min(hardware threads, 16) threads; both are invisible, so a machine where they differ proves the same bytes.)
FRESH = Step(hash=0, q=1, bits=0, K=1, coset=False, D=0, host=1, threads=16, entry="gen_fibsq", seeds="A")
PLAIN = (1, False, 0)


def values(log_n, log_b):
    """factor -> its values for a batch of this shape."""
    return {"hash": (0, 1), "q": (1, 3, MAX_QUERIES), "bits": (0, 6, 12), "K": (1, 2, 3), "coset": (False, True),
            "D": (0, 2, sw.largest_stop(log_n, log_b)), "host": (0, 1), "threads": (1, 4, 16), "entry": ENTRIES, "seeds": ("A", "B")}


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


# ---- the conditions, each on its own --------------------------------------------------------------------------------------------
def all_pairs(vals):
    return {((f, a), (g, b)) for f, g in itertools.combinations(FACTORS, 2) for a in vals[f] for b in vals[g]}


def pairs_of(step):
    return {((f, getattr(step, f)), (g, getattr(step, g))) for f, g in itertools.combinations(FACTORS, 2)}


def all_changes(vals):
    return {(f, a, b) for f in FACTORS for a in vals[f] for b in vals[f] if a != b}


def changes_of(prev, step):
    return {(f, getattr(prev, f), getattr(step, f)) for f in FACTORS if getattr(prev, f) != getattr(step, f)}


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


def twins(steps):
    """Indices i where steps i and i + 1 differ, but in nothing the bytes depend on."""
    return [i for i, (a, b) in enumerate(zip(steps, steps[1:]))
            if a != b and all(getattr(a, f) == getattr(b, f) for f in FACTORS if f not in INVISIBLE)]


FAULT_KINDS = ("plain", "stopped", "coset_k3")


def _fits(kind, s):
    if kind == "plain":
        return sw.fmt(s) == PLAIN
    if kind == "stopped":
        return s.D > 0
    return s.K == 3 and s.coset and s.D == 0


def fault_steps(steps):
    """{index: kind} of the three steps that prove corrupted traces first: the earliest step of index >= 1 that fits each kind (step 0
    is left alone, so that every failed proof happens on a batch that has proved before)."""
    out = {}
    for kind in FAULT_KINDS:
        for i, s in enumerate(steps):
            if i >= 1 and _fits(kind, s) and i not in out:
                out[i] = kind
                break
    return out


def fault_message(step):
    """What zk_batch_prove says about a trace that breaks the constraints (ZK_ERR_CHECK; csrc/batch.hip, prover.rs:238)."""
    return f"final FRI layer has degree >= 2^{step.D}" if step.D else "last FRI layer is not constant"


def broken_proofs(steps, i, log_batch):
    """The proofs whose trace is corrupted before fault step i: proof 1 alone; on the second fault step of the walk two proofs, of which
    the lower one is reported; a batch of one has only proof 0."""
    if log_batch == 0:
        return (0,)
    if sorted(fault_steps(steps)).index(i) == 1:
        return (1, 3) if log_batch >= 2 else (0, 1)
    return (1,)


def unmet(steps, log_n, log_b):
    """Names of the conditions `steps` does not meet."""
    vals = values(log_n, log_b)
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
    if sorted(fault_steps(steps).values()) != sorted(FAULT_KINDS):
        out.append("fault steps")
    if len(twins(steps)) < 2:
        out.append("twins")
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


@functools.lru_cache(maxsize=None)
def walk(log_n, log_b, seed=SEED):
    """The walk for a batch of shape (log_n, log_b), as a tuple of Steps; the batch size changes no step."""
    rng = random.Random(f"batch/{seed}/{log_n}/{log_b}")
    vals = values(log_n, log_b)
    formats = (PLAIN, big_format(log_n, log_b))
    steps = [FRESH]
    pairs, changes = missing_pairs(steps, vals), missing_changes(steps, vals)
    while unmet(steps, log_n, log_b) and len(steps) < MAX_STEPS:
        prev = steps[-1]
        cands = [_random_step(rng, vals, prev) for _ in range(600)]
        cands += [_mutated(rng, vals, prev, FACTORS, rng.randint(1, 5)) for _ in range(200)]
        cands += [_mutated(rng, vals, prev, INVISIBLE, rng.randint(1, 3)) for _ in range(50)]
        need_fault = set(FAULT_KINDS) - set(fault_steps(steps).values())
        split = host_split(steps)
        best, best_score = None, None
        for c in cands:
            score = len(pairs_of(c) & pairs) + 3 * len(changes_of(prev, c) & changes)
            for triple in formats:
                if sw.fmt(c) == triple:
                    if sw.fmt(prev) == triple:
                        score -= 100                         # would spoil an isolated occurrence
                    elif len(sw.isolated(steps, triple)) < 3:
                        score += 40
            if sw.fmt(c) == PLAIN != sw.fmt(prev) and c.hash == 0 and len(split[c.host]) < 2:
                score += 30
            if not largest_decommitment(steps, log_n) and largest_decommitment([c], log_n):
                score += 40
            score += 40 * sum(_fits(k, c) for k in need_fault)
            if len(twins(steps)) < 2 and twins([prev, c]):
                score += 25
            if best_score is None or score > best_score:
                best, best_score = c, score
        steps.append(best)
        pairs -= pairs_of(best)
        changes -= changes_of(prev, best)
    left = unmet(steps, log_n, log_b)
    assert not left, (left, len(steps))
    return tuple(steps)


# ---- the reference proofs -------------------------------------------------------------------------------------------------------
forget_commits = sw.forget_commits


def expected(orc, shape, step, p):
    """The reference proof of proof p of the batch in `step`, for `shape` = (log_n, log_b): stop_ref.stop_proof's .data, .state,
    .public_last, .coef, .c (layers, trees, roots).  Host levels, threads and the trace entry point are not arguments: they must not
    change a byte."""
    log_n, log_b = shape
    with sw._unbounded_commit_cache():
        return stop_ref.stop_proof(orc, log_n, log_b, step.q, step.hash, step.K, step.coset, step.D, step.bits, SEED_SETS[step.seeds] + p)


def bit_flips(shape, i, batch, plen):
    """Step i's three mutations of one of its proofs, [(proof, byte, bit)], drawn from the step's own seeded Random: one in the first
    64 bytes (the first root, the alphas, the second root), one in the middle third, one inside the last 32 bytes (the last digest of
    the last opened path)."""
    rng = random.Random(f"batch flips/{SEED}/{shape[0]}/{shape[1]}/{i}")
    spans = ((0, 64), (plen // 3, 2 * plen // 3), (plen - 32, plen))
    return [(rng.randrange(batch), rng.randrange(lo, hi), rng.randrange(8)) for lo, hi in spans]
