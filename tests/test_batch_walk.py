"""The covering walks of tests/batch_walk.py without a GPU: every covering condition on its own, written without the helper's own
condition functions, and every reference proof of one walk under the plain-Python verifier of tests/stop_ref.py."""
import pytest

import batch_walk as bw
import fold_ref
import stop_ref

SHAPES = [(7, 2), (10, 3), (6, 2)]                           # (log_n, log_b) of tests/test_gpu_batch_walk.py
shape = pytest.mark.parametrize("log_n,log_b", SHAPES)
LARGEST_D = {(7, 2): 6, (10, 3): 8, (6, 2): 5}               # D <= 8, D <= log_n - 1, D + log_b <= 12, worked out by hand


def _format(s):
    return (s.K, s.coset, s.D)


def _apart(steps, triple):
    """Indices of the steps of format `triple` whose neighbours both have another format."""
    return [i for i, s in enumerate(steps) if _format(s) == triple and (i == 0 or _format(steps[i - 1]) != triple)
            and (i + 1 == len(steps) or _format(steps[i + 1]) != triple)]


@shape
def test_steps_take_their_values_from_the_table(log_n, log_b):
    vals = bw.values(log_n, log_b)
    assert set(vals) == set(bw.FACTORS) and len(bw.FACTORS) == 10
    assert vals["D"] == (0, 2, LARGEST_D[(log_n, log_b)])
    assert vals["hash"] == (0, 1)                                                      # BLAKE2s is refused by the batch
    assert vals["q"][-1] == 16                                                         # zk_batch_set_queries' limit
    assert vals["bits"][1] <= 10 < vals["bits"][-1]                                    # the pool grinds 6 bits, the device Grinder 12
    assert max(vals["threads"]) == 16
    for s in bw.walk(log_n, log_b):
        assert all(getattr(s, f) in vals[f] for f in bw.FACTORS), s


@shape
def test_walk_is_deterministic_and_short(log_n, log_b):
    bw.walk.cache_clear()
    first = bw.walk(log_n, log_b)
    bw.walk.cache_clear()
    assert bw.walk(log_n, log_b) == first
    assert isinstance(first, tuple) and len(first) <= bw.MAX_STEPS == 32


@shape
def test_every_pair_of_values_occurs(log_n, log_b):
    steps, vals = bw.walk(log_n, log_b), bw.values(log_n, log_b)
    seen = set()
    for s in steps:
        d = s._asdict()
        seen |= {(f, d[f], g, d[g]) for f in bw.FACTORS for g in bw.FACTORS if f != g}
    want = {(f, a, g, b) for f in bw.FACTORS for g in bw.FACTORS if f != g for a in vals[f] for b in vals[g]}
    assert len(want) == 2 * len(bw.all_pairs(vals)) and not want - seen, sorted(want - seen)[:5]


@shape
def test_every_ordered_change_occurs(log_n, log_b):
    steps, vals = bw.walk(log_n, log_b), bw.values(log_n, log_b)
    seen = {(f, getattr(a, f), getattr(b, f)) for a, b in zip(steps, steps[1:]) for f in bw.FACTORS}
    for f in bw.FACTORS:
        for a in vals[f]:
            for b in vals[f]:
                assert a == b or (f, a, b) in seen, (f, a, b)


@shape
def test_both_corner_formats_recur_apart(log_n, log_b):
    """(1, off, 0) -- the fused launch chain -- and (3, on, largest D) are each left and entered again; of the isolated (1, off, 0)
    steps with SHA-256, two hand tree tops to the host threads and two keep them on the device."""
    steps = bw.walk(log_n, log_b)
    for triple in ((1, False, 0), (3, True, LARGEST_D[(log_n, log_b)])):
        assert len(_apart(steps, triple)) >= 3, triple
    sha = [steps[i] for i in _apart(steps, (1, False, 0)) if steps[i].hash == 0]
    assert sum(s.host == 1 for s in sha) >= 2 and sum(s.host == 0 for s in sha) >= 2


@shape
def test_the_walk_starts_at_the_fresh_batch(log_n, log_b):
    """Step 0 is what zk_batch_create leaves behind, so the first d_work, final-polynomial table, Grinder and regrown gather buffers
    all appear on a batch that has already proved."""
    steps = bw.walk(log_n, log_b)
    s = steps[0]
    assert (s.K, s.coset, s.D, s.q, s.bits, s.hash) == (1, False, 0, 1, 0, 0)
    for first in (lambda t: _format(t) != (1, False, 0), lambda t: t.D > 0, lambda t: t.bits > 10, lambda t: t.q > 1):
        assert min(i for i, t in enumerate(steps) if first(t)) >= 1


@shape
def test_the_largest_decommitment_is_held(log_n, log_b):
    hits = [s for s in bw.walk(log_n, log_b) if s.q == 16 and s.K == 3 and not s.coset and fold_ref.groups(log_n - s.D, 3)[-1][1] < 3]
    assert hits


@shape
def test_fault_steps_fit_their_formats(log_n, log_b):
    steps = bw.walk(log_n, log_b)
    at = bw.fault_steps(steps)
    assert sorted(at.values()) == sorted(bw.FAULT_KINDS) and len(at) == 3 and min(at) >= 1
    fits = {"plain": lambda s: _format(s) == (1, False, 0), "stopped": lambda s: s.D > 0, "coset_k3": lambda s: s.K == 3 and s.coset and s.D == 0}
    for i, kind in at.items():
        assert fits[kind](steps[i]), (i, kind)
        assert not any(fits[kind](s) for s in steps[1:i]), (i, kind)                   # the earliest step that fits
        want = f"final FRI layer has degree >= 2^{steps[i].D}" if kind == "stopped" else "last FRI layer is not constant"
        assert bw.fault_message(steps[i]) == want
    second = sorted(at)[1]
    for i in at:
        assert bw.broken_proofs(steps, i, 0) == (0,)
        assert bw.broken_proofs(steps, i, 1) == ((0, 1) if i == second else (1,))
        assert bw.broken_proofs(steps, i, 2) == ((1, 3) if i == second else (1,))


@shape
def test_twins_differ_only_in_invisible_factors(log_n, log_b):
    steps = bw.walk(log_n, log_b)
    visible = [f for f in bw.FACTORS if f not in ("host", "threads", "entry")]
    at = [i for i, (a, b) in enumerate(zip(steps, steps[1:])) if a != b and all(getattr(a, f) == getattr(b, f) for f in visible)]
    assert len(at) >= 2 and at == bw.twins(steps)


@shape
def test_tree_ids_and_leaf_widths(log_n, log_b):
    """tree_steps against the rules of DESIGN.md 7d written out again: ids 0, 1 and the output of every group but a stopped proof's
    last; with coset leaves the tree over a group's input has 2^steps values per leaf."""
    for s in bw.walk(log_n, log_b):
        got = bw.tree_steps(log_n, s)
        Rp, ids, r0 = log_n - s.D, {0: 0}, 0
        while r0 < Rp:
            ids[1 + r0] = min(s.K, Rp - r0) if s.coset else 0
            r0 += min(s.K, Rp - r0)
        if s.D == 0:
            ids[1 + log_n] = 0
        assert got == ids, s
        assert all(t not in got for t in range(1 + Rp + (s.D == 0), log_n + 2))


def test_seeds_and_bit_flips():
    s = bw.FRESH
    assert bw.seeds_of(s, 4) == ([1, 1, 1, 1], [3141592, 3141593, 3141594, 3141595])
    assert bw.seeds_of(s._replace(seeds="B"), 2) == ([1, 1], [271828, 271829])
    for i in range(8):
        flips = bw.bit_flips((7, 2), i, 4, 3000)
        assert flips == bw.bit_flips((7, 2), i, 4, 3000) and len(flips) == 3
        (p0, b0, _), (p1, b1, _), (p2, b2, _) = flips
        assert 0 <= b0 < 64 and 1000 <= b1 < 2000 and 3000 - 32 <= b2 < 3000
        assert all(0 <= p < 4 and 0 <= bit < 8 for p, _, bit in flips)
    assert bw.bit_flips((7, 2), 0, 4, 3000) != bw.bit_flips((7, 2), 1, 4, 3000)


def test_every_reference_passes_the_python_verifier(orc):
    """The (7, 2) walk, proofs 0 .. 3 of every step (the batch of four of tests/test_gpu_batch_walk.py): the reference agrees with
    itself, strict and lax, before anything is held to it; twins have the same bytes."""
    log_n, log_b = 7, 2
    steps = bw.walk(log_n, log_b)
    try:
        refs = [[bw.expected(orc, (log_n, log_b), s, p) for p in range(4)] for s in steps]
        for s, pair in zip(steps, refs):
            assert len({r.data for r in pair}) == 4
            for ref in pair:
                assert len(ref.data) == stop_ref.proof_len(log_n, log_b, s.q, s.bits, s.K, s.coset, s.D), s
                assert len(ref.coef) == 1 << s.D and set(ref.c.trees) == set(bw.tree_steps(log_n, s)), s
                for state in (ref.state, None):
                    assert stop_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, s.hash, s.q, s.bits, s.K, s.coset, s.D) == 0, s
        for i in bw.twins(steps):
            assert [(r.data, r.state) for r in refs[i]] == [(r.data, r.state) for r in refs[i + 1]], i
    finally:
        bw.forget_commits()
