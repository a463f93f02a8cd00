"""A covering walk through the settings of one live prover context (tests/test_settings_walk.py, tests/test_gpu_settings_walk.py;
DESIGN.md 7d "Reconfiguring a live context").

zk_ctx keeps state from proof to proof (which ids the last proof materialised, the decommitment buffers, the final polynomial, the
grinder, the early-launch and host-tail paths, the staging buffer), so a wrong proof after a setter call shows only on a context that
has proved before in another configuration.  walk(log_n, log_b) is a list of Steps -- one value for every factor of VALUES -- drawn
from a fixed seed and then extended greedily, one step at a time, by the candidate that meets most of the conditions still open:

  * every pair of values of two different factors occurs in some step, except BLAKE2s (hash 2) with ext = 1, which the
    library refuses and no step holds                                                                     (admissible, missing_pairs)
  * every ordered change of one factor from one value to another occurs between two consecutive steps     (missing_changes)
  * the formats (K, coset, D) = (1, off, 0) and (3, on, largest D) each occur three times, isolated       (isolated)
  * some step holds q = 64, K = 3 and a last group shorter than K, with one-value leaves, ext on and no cap: the most words and
    path nodes a proof can fetch                                                                          (largest_decommitment)
  * two isolated (1, off, 0) steps request early launch without checks, two keep SHA-256 tree tops on the host,
    all four in the base field, and one of the gated ones commits caps                                    (fast_paths, gated_with_cap)
  * a (1, off, 0) step in the base field directly after an ext step requests early launch without checks, another keeps SHA-256
    tree tops on the host: both run on the d_layers that zk_ctx_set_ext has just replaced                 (after_ext)
  * (hash 2, ext 0) -> (hash 0 or 1, ext 1) and back occur between consecutive steps: legal in one setter order only   (hash_ext_order)
  * five steps fit a failed proof: (1, off, 0) with checks on; D > 0 without checks; K = 3 with cosets; ext with checks on;
    ext without checks and D = 0                                                                          (fault_steps)
  * two consecutive steps differ in nothing that the proof bytes depend on                                (twins)
  * at most MAX_STEPS steps

The conditions are checked here once (assert in walk) and one by one in tests/test_settings_walk.py.  expected() is the reference
proof of a step, from cap_ref.proof (ext = 0: every hash and cap; with cap 0 the bytes of stop_ref.stop_proof) or ext_ref.proof
(ext = 1); the commit phases of the models are memoised here without a bound, so a walk builds each (hash, K, coset, D, cap, trace,
prefix) once however its steps are ordered."""
import collections
import contextlib
import functools
import itertools
import random

import cap_ref
import coset_ref
import ext_ref
import fold_ref
import stop_ref

MAX_STEPS = 48
SEED = 20261018
PREFIX = b"settings walk: a transcript prefix"
ENTRIES = ("prove_trace", "prove_resident", "prove_channel", "prove_many")
HOST_LEVELS = ("device", "default", "deep")                 # (0, 0); what a fresh context has; (10, 9)
FACTORS = ("hash", "q", "bits", "K", "coset", "D", "host", "early", "checks", "entry", "a1", "cap", "ext")
INVISIBLE = ("host", "early", "checks", "entry")            # must not change a byte (the prefix of prove_channel aside)
Step = collections.namedtuple("Step", FACTORS, defaults=(0, 0))   # cap, ext: what a fresh context has


def largest_stop(log_n, log_b):
    return max(d for d in range(1, stop_ref.MAX_STOP + 1) if stop_ref.admissible(log_n, log_b, d))


def values(log_n, log_b):
    """factor -> its values for a context of this shape."""
    return {"hash": (0, 1, 2), "q": (1, 3, 64), "bits": (0, 6, 12), "K": (1, 2, 3), "coset": (False, True),
            "D": (0, 2, largest_stop(log_n, log_b)), "host": HOST_LEVELS, "early": (False, True), "checks": (False, True),
            "entry": ENTRIES, "a1": (3141592, 7), "cap": (0, 4, 8), "ext": (0, 1)}


def admissible(step):
    """BLAKE2s has no row leaf: zk_ctx_set_ext and zk_ctx_set_hash refuse hash 2 with ext = 1."""
    return not (step.hash == 2 and step.ext == 1)


def host_levels(name, default):
    return {"device": (0, 0), "default": tuple(default), "deep": (10, 9)}[name]


def fmt(step):
    return (step.K, step.coset, step.D)


def short_last_group(log_n, step):
    """The last group of the folded rounds has fewer than K rounds."""
    return fold_ref.groups(log_n - step.D, step.K)[-1][1] < step.K


# ---- the conditions, each on its own --------------------------------------------------------------------------------------------
def all_pairs(vals):
    return {((f, a), (g, b)) for f, g in itertools.combinations(FACTORS, 2) for a in vals[f] for b in vals[g]} - {(("hash", 2), ("ext", 1))}


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
    """{path: indices} of the isolated (1, off, 0) steps in the base field that take the gated launches / hand tree tops (and the FRI
    tail) to the host."""
    at = [i for i in isolated(steps, (1, False, 0)) if steps[i].ext == 0]
    return {"gated": [i for i in at if steps[i].early and not steps[i].checks],
            "host": [i for i in at if steps[i].hash == 0 and steps[i].host != "device"]}


def gated_with_cap(steps):
    """The gated steps of fast_paths that hand their trees over at a cap."""
    return [i for i in fast_paths(steps)["gated"] if steps[i].cap > 0]


def after_ext(steps):
    """{path: indices} of the (1, off, 0) steps in the base field that directly follow an ext step, by the fast path they take."""
    at = [i for i in range(1, len(steps)) if fmt(steps[i]) == (1, False, 0) and steps[i].ext == 0 and steps[i - 1].ext == 1]
    return {"gated": [i for i in at if steps[i].early and not steps[i].checks],
            "host": [i for i in at if steps[i].hash == 0 and steps[i].host != "device"]}


def after_ext_met(steps):
    """Two different steps, one per path."""
    at = after_ext(steps)
    return any(i != j for i in at["gated"] for j in at["host"])


def hash_ext_order(steps):
    """{direction: indices i} where steps i - 1 -> i go (hash 2, ext 0) -> (hash != 2, ext 1) ("to_ext": the hash is set first) or back
    ("to_blake2s": ext is set first)."""
    def blake(s):
        return s.hash == 2 and s.ext == 0

    def ext(s):
        return s.hash != 2 and s.ext == 1
    return {"to_ext": [i for i in range(1, len(steps)) if blake(steps[i - 1]) and ext(steps[i])],
            "to_blake2s": [i for i in range(1, len(steps)) if ext(steps[i - 1]) and blake(steps[i])]}


def largest_decommitment(steps, log_n):
    return [i for i, s in enumerate(steps) if s.q == 64 and s.K == 3 and not s.coset and short_last_group(log_n, s) and s.ext == 1 and s.cap == 0]


def twins(steps):
    """Indices i where steps i and i + 1 differ, but in nothing the bytes depend on."""
    return [i for i, (a, b) in enumerate(zip(steps, steps[1:]))
            if a != b and all(getattr(a, f) == getattr(b, f) for f in FACTORS if f not in INVISIBLE)]


FAULT_KINDS = ("plain_checks", "stopped", "coset_k3", "ext_checks", "ext_plain")


def _fits(kind, s):
    if kind == "plain_checks":
        return fmt(s) == (1, False, 0) and s.checks
    if kind == "stopped":
        return s.D > 0 and not s.checks
    if kind == "ext_checks":
        return s.ext == 1 and s.checks
    if kind == "ext_plain":
        return s.ext == 1 and not s.checks and s.D == 0
    return s.K == 3 and s.coset and s.D == 0


def fault_steps(steps):
    """{index: kind} of the five steps that prove a corrupted trace first: the earliest step that fits each kind."""
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
    (tests/test_gpu_fri_stop.py::test_bad_trace_fails_the_final_degree_check; prover.rs:238).  With ext on the messages are the same:
    prove_ext_rounds holds both planes of cp to the same checkpoint, ext_final_value tests both planes of the last layer."""
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
    if not gated_with_cap(steps):
        out.append("gated with a cap")
    if not largest_decommitment(steps, log_n):
        out.append("largest decommitment")
    if not after_ext_met(steps):
        out.append("after ext")
    if not all(hash_ext_order(steps).values()):
        out.append("hash/ext order")
    if not all(admissible(s) for s in steps):
        out.append("constraint")
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
    while not admissible(s):
        s = Step(*(rng.choice(vals[f]) for f in FACTORS))
    if prev is not None and rng.random() < 0.75:             # the trace mostly alternates: a stale layer is then a wrong layer
        s = s._replace(a1=[a for a in vals["a1"] if a != prev.a1][0])
    return s


def _mutated(rng, vals, prev, factors, count):
    while True:
        s = prev
        for f in rng.sample(factors, count):
            s = s._replace(**{f: rng.choice(vals[f])})
        if admissible(s):
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
        after, after_met, order = after_ext(steps), after_ext_met(steps), hash_ext_order(steps)
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
                if not gated_with_cap(steps) and gated_with_cap([c]):
                    score += 30
            if not largest_decommitment(steps, log_n) and largest_decommitment([c], log_n):
                score += 40
            score += 40 * sum(_fits(k, c) for k in need_fault)
            score += 40 * sum(not at and bool(hash_ext_order([prev, c])[way]) for way, at in order.items())
            if not after_met:
                hit = after_ext([prev, c])
                if (hit["gated"] and (after["host"] or not after["gated"])) or (hit["host"] and (after["gated"] or not after["host"])):
                    score += 40                              # a path not taken yet, or the second step of the two
                elif c.ext == 1 and fmt(c) != (1, False, 0):
                    score += 5                               # the step before one of them
            if not order["to_ext"] and c.hash == 2:
                score += 5                                   # likewise
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
    """While a walk's references are built, the models' `committed` functions are looked up in one unbounded table (what they compute
    is untouched); the modules' own caches come back afterwards."""
    mods = (fold_ref, coset_ref, stop_ref, cap_ref, ext_ref)
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


class Reference:
    """One reference proof, read the same way whichever model built it: .data (the prefix of prove_channel included), .state, .public_last,
    .coef (the words of the final polynomial in wire order: 2^D, or 2 * 2^D with ext), per tree or layer id .layers (id >= 1 with ext: the two
    planes), .trees (whole heaps), .lg, .ce, .caps (the committed bytes; ce = 0: the root), the component-0 raws .alphas and .betas[r0] that
    zk_last_transcript holds, the component-1 raws .ext_challenges in the order of zk_ctx_ext_challenges ([] without ext), and .model,
    the module that built it."""


def _adapt(mod, proof, step):
    cm, out = proof.c, Reference()
    out.model, out.data, out.state, out.public_last, out.coef = mod, proof.data, proof.state, proof.public_last, list(cm.coef)
    out.layers, out.trees, out.lg, out.ce, out.caps = cm.layers, cm.trees, cm.lg, cm.ce, cm.caps
    if step.ext:
        out.alphas, out.betas = cm.alphas[0::2], {r0: b[0] for r0, b in cm.betas.items()}
        out.ext_challenges = cm.alphas[1::2] + [cm.betas[r0][1] for r0 in sorted(cm.betas)]
    else:
        out.alphas, out.betas, out.ext_challenges = list(cm.alphas), dict(cm.betas), []
    return out


def expected(orc, shape, step):
    """The reference proof of `step` on a context of `shape` = (log_n, log_b), as a Reference.  Host levels, early launch, checks and entry
    point are not arguments: they must not change a byte."""
    log_n, log_b = shape
    assert admissible(step), step
    mod = ext_ref if step.ext else cap_ref
    with _unbounded_commit_cache():
        return _adapt(mod, mod.proof(orc, log_n, log_b, step.q, step.hash, step.K, step.coset, step.D, step.cap, step.bits, step.a1, prefix_of(step)), step)


def model_verdict(orc, shape, step, ref, strict):
    """What the plain-Python verifier of the step's model says about the proof behind the prefix (0 = accepted)."""
    log_n, log_b = shape
    data = ref.data[len(prefix_of(step)):]
    return ref.model.verify(orc, data, ref.state if strict else None, log_n, log_b, ref.public_last, step.hash, step.q, step.bits, step.K,
                            step.coset, step.D, step.cap)
