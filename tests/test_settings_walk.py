"""The covering walks of tests/settings_walk.py without a GPU: every covering condition on its own, every reference proof of both
walks under the C verifier, and the factors that must not change a byte not changing one."""
import ctypes as C

import pytest

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
    # the fast paths are taken, left and taken again: early launch needs checks off, host-built tree tops need SHA-256
    plain = [s for s in steps if (s.K, s.coset, s.D) == (1, False, 0)]
    assert sum(s.early and not s.checks for s in plain) >= 2 and sum(s.host != "device" and s.hash == 0 for s in plain) >= 2


@shape
def test_the_largest_decommitment_is_held(log_n, log_b):
    hits = [s for s in sw.walk(log_n, log_b) if s.q == 64 and s.K == 3 and fold_ref.groups(log_n - s.D, 3)[-1][1] < 3]
    assert hits and any(not s.coset for s in hits)


@shape
def test_fault_steps_fit_their_formats(log_n, log_b):
    steps = sw.walk(log_n, log_b)
    at = sw.fault_steps(steps)
    assert sorted(at.values()) == sorted(sw.FAULT_KINDS) and len(at) == 3
    for i, kind in at.items():
        s = steps[i]
        if kind == "plain_checks":
            assert (s.K, s.coset, s.D, s.checks) == (1, False, 0, True)
        elif kind == "stopped":
            assert s.D > 0 and not s.checks and sw.fault_message(s) == f"final FRI layer has degree >= 2^{s.D}"
        else:
            assert s.K == 3 and s.coset


def _accepted(lib, data, state, log_n, log_b, last, s):
    out = C.c_int32(12345)
    rc = lib.zk_verify_stop(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, s.hash, s.q, s.bits, s.K, int(s.coset), s.D, C.byref(out))
    return rc, out.value


@pytest.fixture(scope="module")
def references(orc):
    """shape -> the reference proof of every step (the (10, 3) walk takes the longest: docs/LOG.md)."""
    out = {sh: [sw.expected(orc, sh, s) for s in sw.walk(*sh)] for sh in SHAPES}
    yield out
    sw.forget_commits()


@shape
def test_c_verifier_accepts_every_reference(zk, references, log_n, log_b):
    """Strict and lax, and the length is zk_proof_data_len_stop.  A prove_channel step's transcript starts behind a prefix: its
    proof is what follows the prefix, and only the lax verifier applies (a strict replay starts from the empty channel)."""
    lib = zk.load()
    for s, ref in zip(sw.walk(log_n, log_b), references[(log_n, log_b)]):
        pre = sw.prefix_of(s)
        assert ref.data[:len(pre)] == pre
        data = ref.data[len(pre):]
        assert len(data) == lib.zk_proof_data_len_stop(log_n, log_b, s.q, s.bits, s.K, int(s.coset), s.D) != 0, s
        assert len(ref.coef) == 1 << s.D
        assert _accepted(lib, data, None, log_n, log_b, ref.public_last, s) == (0, 0), s
        if not pre:
            assert _accepted(lib, data, ref.state, log_n, log_b, ref.public_last, s) == (0, 0), s


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
        assert refs[i].c.roots[0] == refs[i + 1].c.roots[0] and refs[i].public_last == refs[i + 1].public_last, i
