"""The covering walks of tests/batch_walk.py without a GPU: every covering condition on its own, written without the helper's own
condition functions, and every reference of one walk -- cap_ref per proof of a zk_batch_prove step, shared_ref / rows_ref for the one
proof of a shared step -- under its plain-Python verifier and under the library's CPU verifier, valid and mutated."""
import ctypes as C

import numpy as np
import pytest

import batch_walk as bw
import cap_ref
import fold_ref
import rows_ref
import shared_ref
import stop_ref

SHAPES = [(7, 2), (10, 3), (6, 2)]                           # (log_n, log_b) of tests/test_gpu_batch_walk.py
shape = pytest.mark.parametrize("log_n,log_b", SHAPES)
LARGEST_D = {(7, 2): 6, (10, 3): 8, (6, 2): 5}               # D <= 8, D <= log_n - 1, D + log_b <= 12, worked out by hand
LOG_BATCHES = {(7, 2): (2, 3), (10, 3): (1,), (6, 2): (0,)}  # the batches tests/test_gpu_batch_walk.py walks: (6, 2) is a batch of one
HOST_SHARE = {(7, 2, 2): 8, (7, 2, 3): 7, (10, 3, 1): 8, (6, 2, 0): 7}   # min(10 - log_batch, 8, L - 1), worked out by hand
ERR_VERIFY = -6


def _shares(log_n, log_b):
    return min(LOG_BATCHES[(log_n, log_b)]) >= 1


def _walk(log_n, log_b):
    return bw.walk(log_n, log_b, _shares(log_n, log_b))


def _values(log_n, log_b):
    return bw.values(log_n, log_b, _shares(log_n, log_b))


def _format(s):
    return (s.K, s.coset, s.D)


def _apart(steps, triple):
    """Indices of the steps of format `triple` whose neighbours both have another format."""
    return [i for i, s in enumerate(steps) if _format(s) == triple and (i == 0 or _format(steps[i - 1]) != triple)
            and (i + 1 == len(steps) or _format(steps[i + 1]) != triple)]


def _kind(s):
    """The verifier's shared setting of a step, as a name."""
    return "plain" if s.call == "each" else "rows" if s.rows else "shared"


@shape
def test_steps_take_their_values_from_the_table(log_n, log_b):
    vals = _values(log_n, log_b)
    assert set(vals) == set(bw.FACTORS) and len(bw.FACTORS) == 13
    assert bw.FACTORS[:10] == ("hash", "q", "bits", "K", "coset", "D", "host", "threads", "entry", "seeds")
    assert vals["D"] == (0, 2, LARGEST_D[(log_n, log_b)])
    assert vals["hash"] == (0, 1)                                                      # BLAKE2s is refused by the batch
    assert vals["q"][-1] == 16                                                         # zk_batch_set_queries' limit
    assert vals["bits"][1] <= 10 < vals["bits"][-1]                                    # the pool grinds 6 bits, the device Grinder 12
    assert max(vals["threads"]) == 16
    assert vals["cap"] == (0, 4, 8) and vals["rows"] == (False, True)
    assert vals["call"] == (("each", "shared") if _shares(log_n, log_b) else ("each",))   # a batch of one refuses zk_batch_prove_shared
    for s in _walk(log_n, log_b):
        assert all(getattr(s, f) in vals[f] for f in bw.FACTORS), s


@shape
def test_walk_is_deterministic_and_short(log_n, log_b):
    bw.walk.cache_clear()
    first = _walk(log_n, log_b)
    bw.walk.cache_clear()
    assert _walk(log_n, log_b) == first
    assert isinstance(first, tuple) and len(first) <= bw.MAX_STEPS == 32


@shape
def test_every_pair_of_values_occurs(log_n, log_b):
    steps, vals = _walk(log_n, log_b), _values(log_n, log_b)
    seen = set()
    for s in steps:
        d = s._asdict()
        seen |= {(f, d[f], g, d[g]) for f in bw.FACTORS for g in bw.FACTORS if f != g}
    want = {(f, a, g, b) for f in bw.FACTORS for g in bw.FACTORS if f != g for a in vals[f] for b in vals[g]}
    assert len(want) == 2 * len(bw.all_pairs(vals)) and not want - seen, sorted(want - seen)[:5]


@shape
def test_every_ordered_change_occurs(log_n, log_b):
    steps, vals = _walk(log_n, log_b), _values(log_n, log_b)
    seen = {(f, getattr(a, f), getattr(b, f)) for a, b in zip(steps, steps[1:]) for f in bw.FACTORS}
    for f in bw.FACTORS:
        for a in vals[f]:
            for b in vals[f]:
                assert a == b or (f, a, b) in seen, (f, a, b)


@shape
def test_both_corner_formats_recur_apart(log_n, log_b):
    """(1, off, 0) -- the fused launch chain -- and (3, on, largest D) are each left and entered again; of the isolated (1, off, 0)
    steps with SHA-256, two hand tree tops to the host threads and two keep them on the device."""
    steps = _walk(log_n, log_b)
    for triple in ((1, False, 0), (3, True, LARGEST_D[(log_n, log_b)])):
        assert len(_apart(steps, triple)) >= 3, triple
    sha = [steps[i] for i in _apart(steps, (1, False, 0)) if steps[i].hash == 0]
    assert sum(s.host == 1 for s in sha) >= 2 and sum(s.host == 0 for s in sha) >= 2


@shape
def test_the_walk_starts_at_the_fresh_batch(log_n, log_b):
    """Step 0 is what zk_batch_create leaves behind, so the first d_work, final-polynomial table, Grinder, regrown gather buffers, cap,
    shared proof and row leaves all appear on a batch that has already proved."""
    steps = _walk(log_n, log_b)
    s = steps[0]
    assert (s.K, s.coset, s.D, s.q, s.bits, s.hash) == (1, False, 0, 1, 0, 0)
    assert (s.cap, s.call, s.rows) == (0, "each", False)
    for first in (lambda t: _format(t) != (1, False, 0), lambda t: t.D > 0, lambda t: t.bits > 10, lambda t: t.q > 1, lambda t: t.cap > 0,
                  lambda t: t.rows):
        assert min(i for i, t in enumerate(steps) if first(t)) >= 1
    if _shares(log_n, log_b):
        assert min(i for i, t in enumerate(steps) if t.call == "shared") >= 1


@shape
def test_the_largest_decommitment_is_held(log_n, log_b):
    hits = [s for s in _walk(log_n, log_b) if s.q == 16 and s.K == 3 and not s.coset and fold_ref.groups(log_n - s.D, 3)[-1][1] < 3]
    assert hits
    if _shares(log_n, log_b):                                 # ... and once as a shared proof with 3M whole f paths per query
        assert [s for s in hits if s.call == "shared" and not s.rows and s.cap == 0]
        assert bw.largest_shared_decommitment(_walk(log_n, log_b), log_n)
    else:
        assert "largest shared decommitment" not in bw.unmet(_walk(log_n, log_b), log_n, log_b, False)


@shape
def test_fault_steps_fit_their_formats(log_n, log_b):
    steps = _walk(log_n, log_b)
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
def test_fault_steps_of_shared_and_capped_proofs(log_n, log_b):
    """The three kinds that came with caps and shared proofs sit beside the three above: each on the earliest step of index >= 1 that fits
    and is not taken, one proof broken, and a shared proof blamed on "some trace of the batch"."""
    steps, shares = _walk(log_n, log_b), _shares(log_n, log_b)
    kinds = bw.fault_kinds(shares)
    assert kinds == ("plain", "stopped", "coset_k3") + (("shared", "shared_rows", "capped") if shares else ("capped",))
    old, at = bw.fault_steps(steps), bw.fault_steps(steps, kinds)
    assert all(at[i] == k for i, k in old.items()) and sorted(at.values()) == sorted(kinds) and min(at) >= 1
    fits = {"shared": lambda s: s.call == "shared" and not s.rows, "shared_rows": lambda s: s.call == "shared" and s.rows,
            "capped": lambda s: s.call == "each" and s.cap > 0}
    taken = set(old)
    for kind in kinds[3:]:
        i = [j for j, k in at.items() if k == kind][0]
        assert fits[kind](steps[i]) and not any(fits[kind](steps[j]) and j not in taken for j in range(1, i)), (i, kind)
        taken.add(i)
        assert bw.broken_proofs(steps, i, 0) == (0,) and bw.broken_proofs(steps, i, 1) == bw.broken_proofs(steps, i, 3) == (1,)
        want = "some trace of the batch" if kind != "capped" else "proof 1 of the batch"
        assert bw.fault_culprit(steps[i], bw.broken_proofs(steps, i, 2)) == want
        assert bw.fault_message(steps[i]) == (f"final FRI layer has degree >= 2^{steps[i].D}" if steps[i].D else "last FRI layer is not constant")
    for i in old:
        assert bw.fault_culprit(steps[i]._replace(call="each"), (1, 3)) == "proof 1 of the batch"


@shape
def test_twins_differ_only_in_invisible_factors(log_n, log_b):
    steps = _walk(log_n, log_b)
    visible = [f for f in bw.FACTORS if f not in ("host", "threads", "entry")]
    at = [i for i, (a, b) in enumerate(zip(steps, steps[1:])) if a != b and all(getattr(a, f) == getattr(b, f) for f in visible)]
    assert len(at) >= 2 and at == bw.twins(steps)


@shape
def test_rows_twins_toggle_rows_under_zk_batch_prove(log_n, log_b):
    """`rows` is one more invisible factor while the call is zk_batch_prove: some consecutive pair of such steps differs in it and in
    nothing else that is visible."""
    steps = _walk(log_n, log_b)
    visible = [f for f in bw.FACTORS if f not in ("host", "threads", "entry", "rows")]
    at = [i for i, (a, b) in enumerate(zip(steps, steps[1:]))
          if a.call == b.call == "each" and a.rows != b.rows and all(getattr(a, f) == getattr(b, f) for f in visible)]
    assert at and at == bw.rows_twins(steps)
    for s in steps:
        assert (bw.visible(s._replace(rows=not s.rows)) == bw.visible(s)) == (s.call == "each"), s
        assert all(bw.visible(s._replace(**{f: v})) == bw.visible(s) for f in ("host", "threads", "entry") for v in _values(log_n, log_b)[f])
    assert "rows twins" in bw.unmet(steps[:at[0] + 1], log_n, log_b, _shares(log_n, log_b))


@shape
def test_tree_ids_and_leaf_widths(log_n, log_b):
    """tree_steps against the rules of DESIGN.md 7d written out again: ids 0, 1 and the output of every group but a stopped proof's
    last; with coset leaves the tree over a group's input has 2^steps values per leaf."""
    for s in _walk(log_n, log_b):
        got = bw.tree_steps(log_n, s)
        Rp, ids, r0 = log_n - s.D, {0: 0}, 0
        while r0 < Rp:
            ids[1 + r0] = min(s.K, Rp - r0) if s.coset else 0
            r0 += min(s.K, Rp - r0)
        if s.D == 0:
            ids[1 + log_n] = 0
        assert got == ids, s
        assert all(t not in got for t in range(1 + Rp + (s.D == 0), log_n + 2))


@shape
def test_calls_follow_each_other_in_the_fused_format(log_n, log_b):
    """call_isolated: a zk_batch_prove in (1, off, 0) directly after a shared proof at least twice, once after row leaves, and a shared
    proof in (1, off, 0) directly after a zk_batch_prove of another format."""
    steps = _walk(log_n, log_b)
    if not _shares(log_n, log_b):
        assert all(s.call == "each" for s in steps) and "call isolated" not in bw.unmet(steps, log_n, log_b, False)
        return
    pairs = list(zip(steps, steps[1:]))
    each_after = [(a, b) for a, b in pairs if a.call == "shared" and b.call == "each" and _format(b) == (1, False, 0)]
    assert len(each_after) >= 2 and any(a.rows for a, _ in each_after)
    assert [(a, b) for a, b in pairs if a.call == "each" and _format(a) != (1, False, 0) and b.call == "shared" and _format(b) == (1, False, 0)]
    got = bw.call_isolated(steps)
    assert len(got["each_after_shared"]) == len(each_after) and bw.call_isolated_goals(steps) == (4, 4)
    cut = got["each_after_shared"][1]                          # without its second such step the condition is open
    assert "call isolated" in bw.unmet(steps[:cut], log_n, log_b, True)


@shape
def test_the_verifier_changes_its_shared_setting_every_way(log_n, log_b):
    """verifier_shared_changes: (log_batch, rows) in a shared step, (0, False) otherwise; all six ordered changes between plain, shared
    and shared with rows, one of them in the same step as a change of the cap."""
    steps = _walk(log_n, log_b)
    for s in steps:
        assert bw.verifier_shared(s, 3) == ((3, s.rows) if s.call == "shared" else (0, False))
    if not _shares(log_n, log_b):
        assert {bw.verifier_shared(s, 0) for s in steps} == {(0, False)}
        return
    seen = [((_kind(a), _kind(b)), a.cap != b.cap) for a, b in zip(steps, steps[1:]) if _kind(a) != _kind(b)]
    assert {k for k, _ in seen} == {(a, b) for a in ("plain", "shared", "rows") for b in ("plain", "shared", "rows") if a != b}
    assert any(with_cap for _, with_cap in seen)
    got = bw.verifier_shared_changes(steps)
    assert all(got.values()) and bw.verifier_shared_goals(steps) == (7, 7)
    last = max(min(v) for v in got.values())                   # the step that closes the last of the seven
    assert "verifier shared changes" in bw.unmet(steps[:last], log_n, log_b, True)


@shape
def test_caps_lie_on_both_sides_of_the_host_share(log_n, log_b):
    """cap_vs_host_share, with the share worked out by hand from DESIGN.md 7f: among the SHA-256 steps whose f stage is as wide as the
    batch, with host levels on and with them off, one has no cap, one a cap below the share and one a cap at or above it."""
    steps, L = _walk(log_n, log_b), log_n + log_b
    for lb in LOG_BATCHES[(log_n, log_b)]:
        h = HOST_SHARE[(log_n, log_b, lb)]
        assert bw.host_share(log_n, log_b, lb) == h
        for host in (0, 1):
            sha = [s for s in steps if s.hash == 0 and s.host == host and not (s.call == "shared" and s.rows)]
            assert [s for s in sha if s.cap == 0], (lb, host)
            assert [s for s in sha if 0 < min(s.cap, L - 1) < h], (lb, host)
            assert [s for s in sha if min(s.cap, L - 1) >= h], (lb, host)
        assert bw.cap_vs_host_share_goals(steps, log_n, log_b, lb) == (6, 6)
    assert bw.host_share(2, 1, 1) == 0 and bw.host_share(20, 4, 6) == 4 and bw.host_share(20, 4, 8) == 0   # two levels are not worth a hand-over
    assert "cap vs host share" in bw.unmet(steps[:3], log_n, log_b, _shares(log_n, log_b))


@shape
def test_cap_8_is_left_and_entered_around_a_rows_proof(log_n, log_b):
    """deep_cap: cap 8 in a zk_batch_prove and in a shared proof without rows; 8 -> smaller -> 8; a shared proof with rows and cap 8 whose
    two neighbours are such steps.  At (7, 2) with eight proofs the f cap is 2^11 digests: the pinned buffer, by the header's rule."""
    steps = _walk(log_n, log_b)
    assert [s for s in steps if s.cap == 8 and s.call == "each"]
    caps = [s.cap for s in steps]
    leave = [i for i in range(1, len(caps)) if caps[i - 1] == 8 and caps[i] < 8]
    assert leave and [i for i in range(1, len(caps)) if caps[i - 1] < 8 and caps[i] == 8 and i > leave[0]]
    if _shares(log_n, log_b):
        assert [s for s in steps if s.cap == 8 and _kind(s) == "shared"]
        assert [i for i in range(1, len(steps) - 1) if steps[i].cap == 8 and _kind(steps[i]) == "rows"
                and all(t.cap == 8 and _kind(t) != "rows" for t in (steps[i - 1], steps[i + 1]))]
        at = bw.deep_cap(steps)["rows_between"][0]
        assert "deep cap" in bw.unmet(steps[:at + 1], log_n, log_b, True)
    assert len(set(bw.deep_cap_goals(steps, _shares(log_n, log_b)))) == 1
    for (n, b, lb, c), words in {(7, 2, 3, 8): 16 + 8 * 2048, (7, 2, 3, 4): 0, (7, 2, 2, 8): 0, (10, 3, 1, 8): 0, (7, 2, 3, 0): 0,
                                 (6, 2, 0, 8): 0, (2, 1, 8, 8): 0, (4, 1, 8, 4): 16 + 8 * 4096}.items():
        assert bw.pinned_cap_words(n, b, lb, c) == words, (n, b, lb, c)


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


def _cpu_check(lib, step, data, state, log_n, log_b, public_last, log_batch):
    """The check number of the library's CPU verifier: zk_verify_cap for a zk_batch_prove step, zk_verify_shared_rows for a shared one."""
    out = C.c_int32(12345)
    tail = (step.hash, step.q, step.bits, step.K, int(step.coset), step.D, step.cap)
    if step.call == "each":
        rc = lib.zk_verify_cap(data, len(data), state, log_n, log_b, public_last, *tail, C.byref(out))
    else:
        arr = np.ascontiguousarray(public_last, dtype=np.uint32)
        rc = lib.zk_verify_shared_rows(data, len(data), state, log_n, log_b, arr.ctypes.data_as(C.c_void_p), log_batch, *tail, int(step.rows), C.byref(out))
    assert rc == (0 if out.value == 0 else ERR_VERIFY), (rc, out.value)
    return out.value


def test_every_reference_passes_the_python_verifier(zk, orc):
    """The (7, 2) walk for the batch of four of tests/test_gpu_batch_walk.py, proofs 0 .. 3 of every zk_batch_prove step and the one
    proof of every shared step: the reference agrees with itself and with the library's CPU verifier, strict and lax, before anything is
    held to it; three mutated copies per step get the same check number from both; twins have the same bytes, and `cap`, `call` and
    (in a shared step) `rows` change them."""
    log_n, log_b, lb = 7, 2, 2
    lib, steps = zk.load(), bw.walk(log_n, log_b, True)
    try:
        refs = [[bw.expected(orc, (log_n, log_b), s, p, lb) for p in range(4 if s.call == "each" else 1)] for s in steps]
        for i, (s, pair) in enumerate(zip(steps, refs)):
            assert len({r.data for r in pair}) == len(pair)
            plen = bw.expected_len((log_n, log_b), s, lb)
            args = (log_n, log_b, s.q, s.bits, s.K, s.coset, s.D, s.cap)
            assert plen == (cap_ref.proof_len(*args) if s.call == "each" else rows_ref.proof_len(*args, lb) if s.rows else shared_ref.proof_len(*args, lb))
            assert plen == lib.zk_proof_data_len_shared_rows(log_n, log_b, s.q, s.bits, s.K, int(s.coset), s.D, s.cap, lb if s.call == "shared" else 0,
                                                             int(s.rows and s.call == "shared")), s
            for p, ref in enumerate(pair):
                assert len(ref.data) == plen, s
                if s.call == "each" and s.cap == 0:          # the anchor the walk had before caps: stop_ref's bytes
                    old = stop_ref.stop_proof(orc, log_n, log_b, s.q, s.hash, s.K, s.coset, s.D, s.bits, bw.SEED_SETS[s.seeds] + p)
                    assert (ref.data, ref.state, ref.public_last) == (old.data, old.state, old.public_last), s
                    assert len(ref.data) == stop_ref.proof_len(log_n, log_b, s.q, s.bits, s.K, s.coset, s.D), s
                    assert set(ref.c.trees) == set(old.c.trees), s
                    for state in (ref.state, None):
                        assert stop_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, s.hash, s.q, s.bits, s.K, s.coset, s.D) == 0, s
                assert len(ref.coef) == 1 << s.D, s
                ids = set(bw.tree_steps(log_n, s))
                assert set(ref.c.trees) == (ids if s.call == "each" else ids - {0}), s
                for state in (ref.state, None):
                    assert bw.model_verdict(orc, (log_n, log_b), s, ref.data, state, ref.public_last, lb) == 0, (s, state is None)
                    assert _cpu_check(lib, s, ref.data, state, log_n, log_b, ref.public_last, lb) == 0, (s, state is None)
            numbers = []
            for p, byte, bit in bw.bit_flips((log_n, log_b), i, len(pair), plen):
                data = bytearray(pair[p].data)
                data[byte] ^= 1 << bit
                for state in (pair[p].state, None):
                    want = bw.model_verdict(orc, (log_n, log_b), s, bytes(data), state, pair[p].public_last, lb)
                    assert _cpu_check(lib, s, bytes(data), state, log_n, log_b, pair[p].public_last, lb) == want, (s, byte, bit, state is None)
                    numbers.append(want)
            assert numbers[-1] != 0 and numbers[-2] != 0, s    # the flipped path digest is rejected, strict or not
        for i in bw.twins(steps) + bw.rows_twins(steps):
            assert [(r.data, r.state) for r in refs[i]] == [(r.data, r.state) for r in refs[i + 1]], i
        for s, pair in zip(steps, refs):                      # every factor the bytes depend on changes them
            others = {"cap": [c for c in (0, 4, 8) if c != s.cap], "call": ["shared" if s.call == "each" else "each"]}
            if s.call == "shared":
                others["rows"] = [not s.rows]
            for f, vals in others.items():
                for v in vals:
                    assert bw.expected(orc, (log_n, log_b), s._replace(**{f: v}), 0, lb).data != pair[0].data, (s, f, v)
            if s.call == "each":
                flipped = bw.expected(orc, (log_n, log_b), s._replace(rows=not s.rows), 0, lb)
                assert (flipped.data, flipped.state) == (pair[0].data, pair[0].state), s
    finally:
        bw.forget_commits()
