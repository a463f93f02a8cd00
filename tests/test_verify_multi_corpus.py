"""The multi-fault corpus (tests/verify_multi_corpus.py) without a GPU: the yardstick of tests/test_gpu_verify_multi.py, and the
proof that the corpus does its job.  For every item of every shape and both hashes the C verifier's number (zk_verify_check,
zk_verify_fold, zk_verify_coset), strict and plain, is the plain-Python verifier's (fold_ref.verify, coset_ref.verify); the Python
verifiers take about a second per shape, so no shape is left to the C verifier alone.

Then the conditions the corpus has to meet for the ordering claim of the device verifier to be tested at all, asserted on the plain
CPU numbers c(A), c(B) of the two single faults and c(AB) of the pair.  They are conditions on the corpus, not measurements of the
code under test: the figures they came out at are in docs/LOG.md."""
import numpy as np
import pytest

import verify_multi_corpus as mc

HASHES = [0, 1]
IDS = {0: "sha256", 1: "field"}


def _shape_id(shape):
    return "-".join(str(x) for x in shape)


def test_shapes_and_classes():
    """Six shapes, every format; per query one class per key position the device can post (the one-value formats: both path
    kinds of every group) and one per path count; pairs and triples alternate between the two valid proofs."""
    assert {s[0] for s in mc.SHAPES} == set(mc.FORMATS)
    for fmt, log_n, log_b, q, g, K in mc.SHAPES:
        table = mc.field_table(fmt, log_n, log_b, q, g, K)
        data = bytes(max(off + size for _, off, size, _ in table))
        cl = mc.fault_classes(fmt, log_n, log_b, q, g, K, data)
        G = len(mc.fold_ref.groups(log_n, K))
        for k in range(q):
            pos = sorted(f.pos for f in cl if f.query == k and f.pos is not None)
            if fmt == "coset":
                assert pos == list(range(4 + 2 * G))
            else:
                assert pos[:5 + G] == list(range(5 + G)) and len(pos) == len(set(pos)) == 5 + 3 * G
        assert len([f for f in cl if f.kind == "global"]) == 7 + 2 * G + (1 if g else 0)
        assert [f.name for f in cl if f.kind == "count"] == [n for n, _, _, kind in table if kind == "count" and n != "nonce"]   # each path count


@pytest.mark.parametrize("hash_kind", HASHES, ids=IDS.values())
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_shape_id)
def test_cpu_verifier_equals_the_reference_on_the_corpus(zk, orc, shape, hash_kind):
    c = mc.corpus(orc, *shape, hash_kind)
    for strict in (True, False):
        got = mc.cpu_numbers(zk.load(), orc, shape, hash_kind, strict)
        want = mc.ref_checks(orc, c.items, *shape, hash_kind, strict)
        bad = [(c.items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
        assert not bad, (strict, bad)
        assert all(got[i] == 0 for i in c.valid)
    print(f"shape {shape} {IDS[hash_kind]}: {len(c.classes[0])} classes, {len(c.items)} items = {len(c.valid)} valid + {len(c.single)} singles + "
          f"{len(c.pairs)} pairs + {len(c.triples)} triples")
    assert len(c.triples) == mc.TRIPLES and len(c.items) == len({it.label for it in c.items})


def _transcript_rank(check, G):
    """Where the Fiat-Shamir replay finds a failure, in its own order: challenge k, the nonce test between the last beta and the
    first query raw, the final state; None for a number that is not the transcript's."""
    if check == -1999:
        return 10**6
    if check == -1998:
        return 3 + G + 0.5
    return -check - 1000 if check <= -1000 else None


def _kernel(check):
    """The kernel that finds a check on the device: the algebra kernel (cp0, a fold comparison) or the paths kernel."""
    if check == -2 or -200 < check <= -100:
        return "algebra"
    if -7 <= check <= -4 or -500 < check <= -300:
        return "paths"
    return None


def _figures(zk, orc, shape, hash_kind):
    """The figures of the conditions for one (shape, hash): a dict of counts over the shape's pairs."""
    c = mc.corpus(orc, *shape, hash_kind)
    plain = mc.cpu_numbers(zk.load(), orc, shape, hash_kind, False)
    strict = mc.cpu_numbers(zk.load(), orc, shape, hash_kind, True)
    G = len(mc.fold_ref.groups(shape[1], shape[5]))
    n = dict(pairs=len(c.pairs), interact=0, cross_query=0, kernels=0, algebra_wins=0, paths_wins=0, count_later=0, count_earlier=0,
             strict_pairs=0, challenge_pairs=0, strict_bad=[])
    for item, p, a, b in c.pairs:
        fa, fb = c.classes[p][a], c.classes[p][b]
        ca, cb, cab = int(plain[c.single[(p, a)]]), int(plain[c.single[(p, b)]]), int(plain[item])
        if cab not in (ca, cb):
            n["interact"] += 1
        if fa.query is not None and fb.query is not None and fa.query != fb.query:
            (fe, ce), (fl, cl) = sorted(((fa, ca), (fb, cb)), key=lambda t: t[0].query)      # the earlier query, the later query
            if fe.pos is not None and fl.pos is not None and fe.pos > fl.pos and ce != cl and ce != 0 and cab == ce:
                n["cross_query"] += 1                                                        # a position-major key reports cl
            if fl.kind == "count" and fe.kind != "count" and ce != 0 and ce != cl and cab == ce:
                n["count_later"] += 1
            if fe.kind == "count" and (cab in (-1, -3) or -300 < cab <= -200):
                n["count_earlier"] += 1
        if fa.query is not None and fa.query == fb.query and {_kernel(ca), _kernel(cb)} == {"algebra", "paths"} and cab in (ca, cb):
            n["kernels"] += 1
            n[_kernel(cab) + "_wins"] += 1
        # strict: a transcript failure wins, and of two the one the replay meets first
        sa, sb, sab = int(strict[c.single[(p, a)]]), int(strict[c.single[(p, b)]]), int(strict[item])
        ranks = [(r, s) for r, s in ((_transcript_rank(sa, G), sa), (_transcript_rank(sb, G), sb)) if r is not None]
        if ranks:
            n["strict_pairs"] += 1
            if sab != min(ranks)[1]:
                n["strict_bad"].append((c.items[item].label, sa, sb, sab))
            if all(-1998 < s <= -1000 for s in (sa, sb)):
                n["challenge_pairs"] += 1
    return n


_figs = {}


@pytest.fixture(scope="module")
def figures(zk, orc):
    def get(shape, hash_kind):
        if (shape, hash_kind) not in _figs:
            _figs[(shape, hash_kind)] = _figures(zk, orc, shape, hash_kind)
        return _figs[(shape, hash_kind)]
    return get


@pytest.mark.parametrize("hash_kind", HASHES, ids=IDS.values())
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_shape_id)
def test_faults_rarely_interact_and_the_transcript_wins(figures, shape, hash_kind):
    """Per shape: at most 5 % of the pairs have c(AB) outside {c(A), c(B)}; in strict mode every pair with a transcript-visible
    fault reports the transcript's number, of two the one the replay meets first (two challenge fields: the earlier challenge)."""
    n = figures(shape, hash_kind)
    print(f"shape {shape} {IDS[hash_kind]}: " + ", ".join(f"{k} {v}" for k, v in n.items() if k != "strict_bad"))
    assert n["interact"] <= 0.05 * n["pairs"]
    assert not n["strict_bad"], n["strict_bad"][:20]
    assert n["strict_pairs"] >= n["pairs"] - 1 and n["challenge_pairs"] >= 10      # all but (public_last, nothing in the transcript)


@pytest.mark.parametrize("hash_kind", HASHES, ids=IDS.values())
@pytest.mark.parametrize("fmt", mc.FORMATS)
def test_the_corpus_separates_the_orders(figures, fmt, hash_kind):
    """Per format (the sum over its shapes, for each hash): at least 50 pairs with the faults in different queries where the
    CPU reports the fault of the EARLIER query at the LATER position (a position-major key reports the other one); at least 50
    pairs inside one query with one fault found by the algebra kernel and the other by the paths kernel, at least 20 with each
    as the winner; at least 20 pairs of a broken path count in query b with another fault in a query a < b where the CPU reports
    the fault of query a; at least 20 of a broken count in query a with a fault in a query b > a where it reports -3,
    -(200 + j) or -1."""
    tot = {}
    for shape in mc.SHAPES:
        if shape[0] == fmt:
            for k, v in figures(shape, hash_kind).items():
                if k != "strict_bad":
                    tot[k] = tot.get(k, 0) + v
    print(f"format {fmt} {IDS[hash_kind]}: " + ", ".join(f"{k} {v}" for k, v in tot.items()))
    assert tot["cross_query"] >= 50
    assert tot["kernels"] >= 50 and tot["algebra_wins"] >= 20 and tot["paths_wins"] >= 20
    assert tot["count_later"] >= 20
    assert tot["count_earlier"] >= 20
