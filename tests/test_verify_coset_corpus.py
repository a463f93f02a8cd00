"""The tamper corpus of proofs with coset leaves (tests/verify_coset_corpus.py) without a GPU: its field table covers the wire
format, the CPU verifier zk_verify_coset gives every item the number of the plain-Python verifier of tests/coset_ref.py, strict
and plain and for both hashes, and the corpus reaches every check a fixed-layout coset proof can fail and every slot rotation."""
import numpy as np
import pytest

import coset_ref
import fold_ref
import verify_coset_corpus

# (log_n, log_b, q, grind bits, K): groups of 2+2+1; 3+2 with a nonce and seven queries; 3+3+1 on a 2-value last layer; K = 1 at
# the reference's size (ten groups of two slots); 3+1 with three queries
SHAPES = [(5, 2, 2, 0, 2), (5, 2, 7, 8, 3), (7, 1, 1, 0, 3), (10, 3, 1, 0, 1), (4, 1, 3, 0, 3)]


def test_field_table_covers_the_length():
    for log_n in range(2, 11):
        for K in (1, 2, 3):
            for g in (0, 8):
                for q in (1, 3):
                    table = verify_coset_corpus.fields(log_n, 2, q, g, K)         # asserts that the fields end at proof_len
                    spans = sorted((off, off + size) for _, off, size, _ in table)
                    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (log_n, K, g, q)   # no two fields overlap
                    names = [n for n, _, _, _ in table]
                    assert len(set(names)) == len(names)
                    grp = fold_ref.groups(log_n, K)
                    assert len(table) == 6 + 2 * len(grp) + (1 if g else 0) + q + q * (9 + sum((1 << s) + 2 for _, s in grp))


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K", SHAPES)
def test_cpu_verifier_equals_the_reference_on_the_corpus(zk, orc, log_n, log_b, q, g, K, hash_kind):
    lib = zk.load()
    items = verify_coset_corpus.corpus(orc, log_n, log_b, q, g, K, hash_kind)
    G = len(fold_ref.groups(log_n, K))
    for strict in (True, False):
        got = verify_coset_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, hash_kind, strict)
        want = np.array([coset_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K)
                         for it in items], dtype=np.int32)
        bad = [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
        assert not bad, (strict, bad)
        print(f"shape {(log_n, log_b, q, g, K)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
              f"{len(set(want.tolist()))} distinct check numbers")
        assert want[0] == 0                                              # p0.valid
        assert (want != 0).sum() > len(items) // 2                       # mostly rejections
        if not strict:
            # every check a coset proof on the fixed layout can fail: a tampered f value fails -2 first, every group has a slot
            # that is not its value 0 (its fold comparison) and one path
            need = {-2, -4, -5, -6} | {-(100 + j) for j in range(G)} | {-(300 + j) for j in range(G)}
            assert need <= set(want.tolist()), sorted(need - set(want.tolist()))


def test_the_valid_proofs_exercise_every_rotation(orc):
    """K = 3, q = 7, two proofs: in at least one full group (s = 8) the query indices put value 0 in every slot 0..7."""
    log_n, log_b, q, g, K = SHAPES[1]
    assert K == 3 and q >= 7
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    seen = {}
    for hash_kind in (0, 1):
        for r in verify_coset_corpus.ref_objects(orc, log_n, log_b, q, g, K, hash_kind):
            for raw in r.raws:
                tp = raw % (N - 2 * B)
                for j, (r0, steps) in enumerate(fold_ref.groups(log_n, K)):
                    if steps == 3:
                        size = N >> r0
                        seen.setdefault((hash_kind, j), set()).add((tp % size) // (size // 8))
    assert seen
    for hash_kind in (0, 1):
        full = [rots for (h, j), rots in seen.items() if h == hash_kind]
        assert any(rots == set(range(8)) for rots in full), (hash_kind, seen)
