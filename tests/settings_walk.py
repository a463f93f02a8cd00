"""A covering walk through the settings of one live prover context (tests/test_settings_walk.py, tests/test_gpu_settings_walk.py;
DESIGN.md 7d "Reconfiguring a live context").

zk_ctx keeps state from proof to proof (which ids the last proof materialised, the decommitment buffers, the final polynomial, the
grinder, the early-launch and host-tail paths, the staging buffer), so a wrong proof after a setter call shows only on a context that
has proved before in another configuration.  walk(log_n, log_b) is a list of Steps -- one value for every factor of VALUES -- drawn
from a fixed seed and then extended greedily, one step at a time, by the candidate that meets most of the conditions still open:

  * every pair of values of two different factors occurs in some step                                     (missing_pairs)
  * every ordered change of one factor from one value to another occurs between two consecutive steps     (missing_changes)
  * the formats (K, coset, D) = (1, off, 0) and (3, on, largest D) each occur three times, isolated       (isolated)
  * some step holds q = 64, K = 3 and a last group shorter than K, with one-value leaves                  (largest_decommitment)
  * two isolated (1, off, 0) steps request early launch without checks, two keep SHA-256 tree tops on the host    (fast_paths)
  * three steps fit a failed proof: (1, off, 0) with checks on; D > 0 without checks; K = 3 with cosets   (fault_steps)
  * two consecutive steps differ in nothing that the proof bytes depend on                                (twins)
  * at most MAX_STEPS steps

The conditions are checked here once (assert in walk) and one by one in tests/test_settings_walk.py.  expected() is the reference
proof of a step, from stop_ref.stop_proof; the commit phases of fold_ref / coset_ref / stop_ref are memoised here without a bound,
so a walk builds each (hash, K, coset, D, trace, prefix) once however its steps are ordered."""
import collections
import contextlib
import functools
import itertools
import random

import coset_ref
import fold_ref
import stop_ref

MAX_STEPS = 48
SEED = 20261018
PREFIX = b"settings walk: a transcript prefix"
ENTRIES = ("prove_trace", "prove_resident", "prove_channel", "prove_many")
HOST_LEVELS = ("device", "default", "deep")                 # (0, 0); what a fresh context has; (10, 9)
FACTORS = ("hash", "q", "bits", "K", "coset", "D", "host", "early", "checks", "entry", "a1")
INVISIBLE = ("host", "early", "checks", "entry")            # must not change a byte (the prefix of prove_channel aside)
Step = collections.namedtuple("Step", FACTORS)


def largest_stop(log_n, log_b):
    return max(d for d in range(1, stop_ref.MAX_STOP + 1) if stop_ref.admissible(log_n, log_b, d))


def values(log_n, log_b):
    """factor -> its values for a context of this shape."""
    return {"hash": (0, 1), "q": (1, 3, 64), "bits": (0, 6, 12), "K": (1, 2, 3), "coset": (False, True),
            "D": (0, 2, largest_stop(log_n, log_b)), "host": HOST_LEVELS, "early": (False, True), "checks": (False, True),
            "entry": ENTRIES, "a1": (3141592, 7)}


def host_levels(name, default):
    return {"device": (0, 0), "default": tuple(default), "deep": (10, 9)}[name]


def fmt(step):
    return (step.K, step.coset, step.D)


def short_last_group(log_n, step):
    """The last group of the folded rounds has fewer than K rounds."""
    return fold_ref.groups(log_n - step.D, step.K)[-1][1] < step.K


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


def isolated(steps, triple):
    """Indices of the steps of format `triple` with no neighbour of the same format."""
    return [i for i, s in enumerate(steps) if fmt(s) == triple
            and (i == 0 or fmt(steps[i - 1]) != triple) and (i + 1 == len(steps) or fmt(steps[i + 1]) != triple)]


def fast_paths(steps):
    """{path: indices} of the isolated (1, off, 0) steps that take the gated launches / hand tree tops (and the FRI tail) to the host."""
    at = isolated(steps, (1, False, 0))
    return {"gated": [i for i in at if steps[i].early and not steps[i].checks],
            "host": [i for i in at if steps[i].hash == 0 and steps[i].host != "device"]}


def largest_decommitment(steps, log_n):
    return [i for i, s in enumerate(steps) if s.q == 64 and s.K == 3 and not s.coset and short_last_group(log_n, s)]


def twins(steps):
    """Indices i where steps i and i + 1 differ, but in nothing the bytes depend on."""
    return [i for i, (a, b) in enumerate(zip(steps, steps[1:]))
            if a != b and all(getattr(a, f) == getattr(b, f) for f in FACTORS if f not in INVISIBLE)]


FAULT_KINDS = ("plain_checks", "stopped", "coset_k3")


def _fits(kind, s):
    if kind == "plain_checks":
        return fmt(s) == (1, False, 0) and s.checks
    if kind == "stopped":
        return s.D > 0 and not s.checks
    return s.K == 3 and s.coset and s.D == 0


def fault_steps(steps):
    """{index: kind} of the three steps that prove a corrupted trace first: the earliest step that fits each kind."""
    out = {}
    for kind in FAULT_KINDS:
        for i, s in enumerate(steps):
            if _fits(kind, s) and i not in out:
                out[i] = kind
                break
    return out


def fault_message(step):
    """What the library says about a corrupted trace in this step's configuration (ZK_ERR_CHECK in every case): with the self-checks
    the first violated checkpoint (tests/test_gpu_kernels.py::test_reference_self_checks), else the last layer's test
    (tests/test_gpu_fri_stop.py::test_bad_trace_fails_the_final_degree_check; prover.rs:238)."""
    if step.checks:
        return "prover.rs:148-159/:169"
    return f"final FRI layer has degree >= 2^{step.D}" if step.D else "last FRI layer is not constant"


def unmet(steps, log_n, log_b):
    """Names of the conditions `steps` does not meet."""
    vals = values(log_n, log_b)
    out = []
    if missing_pairs(steps, vals):
        out.append("pairs")
    if missing_changes(steps, vals):
        out.append("changes")
    for triple in ((1, False, 0), (3, True, vals["D"][-1])):
        if len(isolated(steps, triple)) < 3:
            out.append(f"format {triple}")
    if min(len(v) for v in fast_paths(steps).values()) < 2:
        out.append("fast paths")
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
def _random_step(rng, vals, prev=None):
    s = Step(*(rng.choice(vals[f]) for f in FACTORS))
    if prev is not None and rng.random() < 0.75:             # the trace mostly alternates: a stale layer is then a wrong layer
        s = s._replace(a1=[a for a in vals["a1"] if a != prev.a1][0])
    return s


def _mutated(rng, vals, prev, factors, count):
    s = prev
    for f in rng.sample(factors, count):
        s = s._replace(**{f: rng.choice(vals[f])})
    return s


@functools.lru_cache(maxsize=None)
def walk(log_n, log_b, seed=SEED):
    """The walk for a context of shape (log_n, log_b), as a tuple of Steps."""
    rng = random.Random(f"{seed}/{log_n}/{log_b}")
    vals = values(log_n, log_b)
    big = (3, True, vals["D"][-1])
    steps = [_random_step(rng, vals)]
    while len(steps) < 6:
        steps.append(_random_step(rng, vals, steps[-1]))
    pairs, changes = missing_pairs(steps, vals), missing_changes(steps, vals)
    while unmet(steps, log_n, log_b) and len(steps) < MAX_STEPS:
        prev = steps[-1]
        cands = [_random_step(rng, vals, prev) for _ in range(600)]
        cands += [_mutated(rng, vals, prev, FACTORS, rng.randint(1, 5)) for _ in range(200)]
        cands += [_mutated(rng, vals, prev, INVISIBLE, rng.randint(1, 4)) for _ in range(50)]
        need_fault = set(FAULT_KINDS) - set(fault_steps(steps).values())
        best, best_score = None, -1
        for c in cands:
            score = len(pairs_of(c) & pairs) + 3 * len(changes_of(prev, c) & changes)
            for triple in ((1, False, 0), big):
                if fmt(c) == triple:
                    if fmt(prev) == triple:
                        score -= 100                         # would spoil an isolated occurrence
                    elif len(isolated(steps, triple)) < 3:
                        score += 40
            if fmt(c) == (1, False, 0) != fmt(prev):
                score += 30 * sum(len(at) < 2 and bool(fast_paths([c])[path]) for path, at in fast_paths(steps).items())
            if not largest_decommitment(steps, log_n) and largest_decommitment([c], log_n):
                score += 40
            score += 40 * sum(_fits(k, c) for k in need_fault)
            if len(twins(steps)) < 2 and twins([prev, c]):
                score += 25
            if score > best_score:
                best, best_score = c, score
        steps.append(best)
        pairs -= pairs_of(best)
        changes -= changes_of(prev, best)
    left = unmet(steps, log_n, log_b)
    assert not left, (left, len(steps))
    return tuple(steps)


# ---- the reference proofs -------------------------------------------------------------------------------------------------------
_COMMITS = {}


def _memoised(mod):
    raw = mod.committed.__wrapped__                          # the function under the module's own small lru_cache

    def committed(*args):
        key = (mod.__name__,) + args
        if key not in _COMMITS:
            _COMMITS[key] = raw(*args)
        return _COMMITS[key]
    return committed


@contextlib.contextmanager
def _unbounded_commit_cache():
    """While a walk's references are built, the three `committed` functions are looked up in one unbounded table (what they compute is
    untouched); the modules' own caches come back afterwards."""
    mods = (fold_ref, coset_ref, stop_ref)
    saved = [m.committed for m in mods]
    for m in mods:
        m.committed = _memoised(m)
    try:
        yield
    finally:
        for m, f in zip(mods, saved):
            m.committed = f


def forget_commits():
    _COMMITS.clear()


def prefix_of(step):
    return PREFIX if step.entry == "prove_channel" else b""


def expected(orc, shape, step):
    """The reference proof of `step` on a context of `shape` = (log_n, log_b): stop_ref.stop_proof's .data (the prefix of prove_channel
    included), .state, .coef, .c.  Host levels, early launch, checks and entry point are not arguments: they must not change a byte."""
    log_n, log_b = shape
    with _unbounded_commit_cache():
        return stop_ref.stop_proof(orc, log_n, log_b, step.q, step.hash, step.K, step.coset, step.D, step.bits, step.a1, prefix_of(step))
