"""The covering walks of tests/settings_walk.py without a GPU: every covering condition on its own, every reference proof of both
walks under the C verifier and under its model's plain-Python verifier, the factors that must not change a byte not changing one, and
cap, ext and hash each changing some."""
import ctypes as C

import pytest

import cap_ref
import ext_ref
import fold_ref
import settings_walk as sw

SHAPES = [(6, 3), (10, 3)]
shape = pytest.mark.parametrize("log_n,log_b", SHAPES)


@shape
def test_steps_take_their_values_from_the_table(log_n, log_b):
    vals = sw.values(log_n, log_b)
    assert vals["D"] == {(6, 3): (0, 2, 5), (10, 3): (0, 2, 8)}[(log_n, log_b)]       # the largest admissible stop, worked out by hand
    assert vals["bits"][-1] > 10 >= vals["bits"][1]                                    # 12 is the grinder's first allocation
    for s in sw.walk(log_n, log_b):
        assert all(getattr(s, f) in vals[f] for f in sw.FACTORS), s


@shape
def test_walk_is_deterministic_and_short(log_n, log_b):
    sw.walk.cache_clear()
    first = sw.walk(log_n, log_b)
    sw.walk.cache_clear()
    assert sw.walk(log_n, log_b) == first
    assert len(first) <= sw.MAX_STEPS == 48


@shape
def test_every_pair_of_values_occurs(log_n, log_b):
    steps, vals = sw.walk(log_n, log_b), sw.values(log_n, log_b)
    seen = set()
    for s in steps:
        d = s._asdict()
        seen |= {(f, d[f], g, d[g]) for f in sw.FACTORS for g in sw.FACTORS if f != g}
    want = {(f, a, g, b) for f in sw.FACTORS for g in sw.FACTORS if f != g for a in vals[f] for b in vals[g]}
    want -= {("hash", 2, "ext", 1), ("ext", 1, "hash", 2)}                             # the one pair the library refuses
    assert {"cap", "ext"} <= set(sw.FACTORS) and vals["hash"] == (0, 1, 2) and vals["cap"] == (0, 4, 8) and vals["ext"] == (0, 1)
    assert not {"cap", "ext", "hash"} & set(sw.INVISIBLE)
    assert len(want) == 2 * len(sw.all_pairs(vals)) and not want - seen, sorted(want - seen)[:5]


@shape
def test_every_ordered_change_occurs(log_n, log_b):
    steps, vals = sw.walk(log_n, log_b), sw.values(log_n, log_b)
    seen = {(f, getattr(a, f), getattr(b, f)) for a, b in zip(steps, steps[1:]) for f in sw.FACTORS}
    for f in sw.FACTORS:
        for a in vals[f]:
            for b in vals[f]:
                assert a == b or (f, a, b) in seen, (f, a, b)


@shape
def test_both_corner_formats_recur_apart(log_n, log_b):
    """(1, off, 0) -- the only format on the gated and host-tail paths -- and (3, on, largest D) are each left and entered again."""
    steps = sw.walk(log_n, log_b)
    for triple in ((1, False, 0), (3, True, sw.largest_stop(log_n, log_b))):
        at = [i for i, s in enumerate(steps) if (s.K, s.coset, s.D) == triple]
        assert len(at) >= 3 and all(b - a > 1 for a, b in zip(at, at[1:])), (triple, at)
    # the fast paths are taken, left and taken again: early launch needs checks off, host-built tree tops need SHA-256, both the base field
    plain = [s for s in steps if (s.K, s.coset, s.D, s.ext) == (1, False, 0, 0)]
    assert sum(s.early and not s.checks for s in plain) >= 2 and sum(s.host != "device" and s.hash == 0 for s in plain) >= 2
    assert any(s.early and not s.checks and s.cap > 0 for s in plain) and sw.gated_with_cap(steps)     # the gated launches hand over at a cap


@shape
def test_the_largest_decommitment_is_held(log_n, log_b):
    hits = [s for s in sw.walk(log_n, log_b) if s.q == 64 and s.K == 3 and fold_ref.groups(log_n - s.D, 3)[-1][1] < 3]
    assert hits and any(not s.coset for s in hits)
    assert any(not s.coset and s.ext == 1 and s.cap == 0 for s in hits)                # two words per value, whole paths: the most a proof fetches
    assert sw.largest_decommitment(sw.walk(log_n, log_b), log_n)


@shape
def test_no_step_holds_blake2s_with_ext(log_n, log_b):
    steps = sw.walk(log_n, log_b)
    assert not any(s.hash == 2 and s.ext == 1 for s in steps)
    assert any(s.hash == 2 for s in steps) and any(s.ext == 1 for s in steps)
    assert not sw.admissible(steps[0]._replace(hash=2, ext=1)) and sw.admissible(steps[0]._replace(hash=2, ext=0))
    assert (("hash", 2), ("ext", 1)) not in sw.all_pairs(sw.values(log_n, log_b))


@shape
def test_plain_steps_follow_ext_steps_on_both_fast_paths(log_n, log_b):
    """zk_ctx_set_ext replaces d_layers; the next base-field proof takes the gated launches, another one the host tree tops and FRI tail."""
    steps = sw.walk(log_n, log_b)
    after = [i for i in range(1, len(steps)) if steps[i - 1].ext == 1 and steps[i].ext == 0 and (steps[i].K, steps[i].coset, steps[i].D) == (1, False, 0)]
    gated = [i for i in after if steps[i].early and not steps[i].checks]
    host = [i for i in after if steps[i].hash == 0 and steps[i].host != "device"]
    assert len(after) >= 2 and any(i != j for i in gated for j in host), (after, gated, host)
    assert sw.after_ext(steps) == {"gated": gated, "host": host} and sw.after_ext_met(steps)


@shape
def test_blake2s_and_ext_follow_each_other_both_ways(log_n, log_b):
    steps = sw.walk(log_n, log_b)
    ways = sw.hash_ext_order(steps)
    assert ways["to_ext"] and ways["to_blake2s"]
    for i in ways["to_ext"]:
        assert (steps[i - 1].hash, steps[i - 1].ext, steps[i].ext) == (2, 0, 1) and steps[i].hash in (0, 1)
    for i in ways["to_blake2s"]:
        assert (steps[i].hash, steps[i].ext, steps[i - 1].ext) == (2, 0, 1) and steps[i - 1].hash in (0, 1)


@shape
def test_fault_steps_fit_their_formats(log_n, log_b):
    steps = sw.walk(log_n, log_b)
    at = sw.fault_steps(steps)
    assert sorted(at.values()) == sorted(sw.FAULT_KINDS) and len(at) == 5
    assert set(sw.FAULT_KINDS) == {"plain_checks", "stopped", "coset_k3", "ext_checks", "ext_plain"}
    for i, kind in at.items():
        s = steps[i]
        if kind == "plain_checks":
            assert (s.K, s.coset, s.D, s.checks) == (1, False, 0, True)
        elif kind == "stopped":
            assert s.D > 0 and not s.checks and sw.fault_message(s) == f"final FRI layer has degree >= 2^{s.D}"
        elif kind == "ext_checks":                            # prove_ext_rounds: the cp checkpoint on both planes
            assert s.ext == 1 and s.checks and sw.fault_message(s) == "prover.rs:148-159/:169"
        elif kind == "ext_plain":                             # ext_final_value: both planes of the last layer
            assert s.ext == 1 and not s.checks and s.D == 0 and sw.fault_message(s) == "last FRI layer is not constant"
        else:
            assert s.K == 3 and s.coset


def _accepted(lib, data, state, log_n, log_b, last, s):
    out = C.c_int32(12345)
    rc = lib.zk_verify_ext(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, s.hash, s.q, s.bits, s.K, int(s.coset), s.D, s.cap, s.ext, C.byref(out))
    return rc, out.value


@pytest.fixture(scope="module")
def references(orc):
    """shape -> the reference proof of every step (the (10, 3) walk takes the longest: docs/LOG.md)."""
    out = {sh: [sw.expected(orc, sh, s) for s in sw.walk(*sh)] for sh in SHAPES}
    yield out
    sw.forget_commits()


@shape
def test_c_verifier_accepts_every_reference(zk, orc, references, log_n, log_b):
    """Strict and lax, and the length is zk_proof_data_len_ext; the plain-Python verifier of the step's model answers 0 too.  A prove_channel step's transcript starts behind a prefix: its
    proof is what follows the prefix, and only the lax verifier applies (a strict replay starts from the empty channel)."""
    lib = zk.load()
    for s, ref in zip(sw.walk(log_n, log_b), references[(log_n, log_b)]):
        pre = sw.prefix_of(s)
        assert ref.data[:len(pre)] == pre
        data = ref.data[len(pre):]
        assert len(data) == lib.zk_proof_data_len_ext(log_n, log_b, s.q, s.bits, s.K, int(s.coset), s.D, s.cap, s.ext) != 0, s
        assert len(ref.coef) == 1 << (s.D + s.ext)
        assert ref.model is (ext_ref if s.ext else cap_ref)
        assert _accepted(lib, data, None, log_n, log_b, ref.public_last, s) == (0, 0), s
        assert sw.model_verdict(orc, (log_n, log_b), s, ref, strict=False) == 0, s
        if not pre:
            assert _accepted(lib, data, ref.state, log_n, log_b, ref.public_last, s) == (0, 0), s
            assert sw.model_verdict(orc, (log_n, log_b), s, ref, strict=True) == 0, s


@shape
def test_visible_factors_change_bytes(orc, references, log_n, log_b):
    """cap, ext and hash each moved to another admissible value give another proof: a library that ignores one of the three setters
    cannot pass the GPU walk.  (With BLAKE2s ext has no other admissible value.)"""
    steps, refs, vals = sw.walk(log_n, log_b), references[(log_n, log_b)], sw.values(log_n, log_b)
    moved = 0
    for i, (s, ref) in enumerate(zip(steps, refs)):
        for f in ("cap", "ext", "hash"):
            others = [t for t in (s._replace(**{f: v}) for v in vals[f] if v != getattr(s, f)) if sw.admissible(t)]
            if not others:
                assert f == "ext" and s.hash == 2, (i, f)
                continue
            other = others[i % len(others)]
            assert sw.expected(orc, (log_n, log_b), other).data != ref.data, (i, f, other)
            moved += 1
    assert moved >= 3 * len(steps) - sum(s.hash == 2 for s in steps)


@shape
def test_invisible_factors_change_no_byte(references, log_n, log_b):
    steps, refs = sw.walk(log_n, log_b), references[(log_n, log_b)]
    at = sw.twins(steps)
    assert len(at) >= 2
    for i in at:
        a, b = steps[i], steps[i + 1]
        assert a != b and all(getattr(a, f) == getattr(b, f) for f in sw.FACTORS if f not in sw.INVISIBLE)
        if sw.prefix_of(a) == sw.prefix_of(b):
            assert (refs[i].data, refs[i].state) == (refs[i + 1].data, refs[i + 1].state), i
        # across a prefix the challenges differ; what is committed before the first challenge does not
        assert refs[i].caps[0] == refs[i + 1].caps[0] and refs[i].public_last == refs[i + 1].public_last, i
        assert len(refs[i].caps[0]) == 32 << min(a.cap, log_n + log_b - 1) and refs[i].ce[0] == refs[i + 1].ce[0]
