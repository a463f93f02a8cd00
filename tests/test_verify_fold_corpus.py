"""The tamper corpus of folded proofs (tests/verify_fold_corpus.py) without a GPU: its field table covers the wire format, the
CPU verifier zk_verify_fold gives every item the number of the plain-Python verifier of tests/fold_ref.py, the corpus is not
trivial, and the null-handle answers of zk_verifier_set_fold / zk_verifier_get_fold."""
import numpy as np
import pytest

import fold_ref
import verify_fold_corpus

# (log_n, log_b, q, grind bits, K): groups of 2+2+1, 3+2 with a nonce, 3+3+1 on a 2-value last layer, and the reference's size
SHAPES = [(5, 2, 2, 0, 2), (5, 2, 2, 8, 3), (7, 1, 1, 0, 3), (10, 3, 1, 0, 2)]


def test_field_table_covers_the_length():
    for log_n in range(2, 11):
        for K in (1, 2, 3):
            for g in (0, 8):
                for q in (1, 3):
                    table = verify_fold_corpus.fields(log_n, 2, q, g, K)          # asserts that the fields end at proof_len
                    spans = sorted((off, off + size) for _, off, size, _ in table)
                    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (log_n, K, g, q)   # no two fields overlap
                    names = [n for n, _, _, _ in table]
                    assert len(set(names)) == len(names)
                    G = len(fold_ref.groups(log_n, K))
                    opened = sum(1 << s for _, s in fold_ref.groups(log_n, K))
                    assert len(table) == 6 + 2 * G + (1 if g else 0) + q + q * (12 + 3 * opened)


@pytest.mark.parametrize("log_n,log_b,q,g,K", SHAPES)
def test_cpu_verifier_equals_the_reference_on_the_corpus(zk, orc, log_n, log_b, q, g, K):
    lib = zk.load()
    items = verify_fold_corpus.corpus(orc, log_n, log_b, q, g, K, 0)
    for strict in (True, False):
        got = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, 0, strict)
        want = np.array([fold_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, 0, q, g, K) for it in items],
                        dtype=np.int32)
        bad = [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
        assert not bad, (strict, bad)
        print(f"shape {(log_n, log_b, q, g, K)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
              f"{len(set(want.tolist()))} distinct check numbers")
        assert want[0] == 0                                              # p0.valid
        if strict:
            assert (want != 0).sum() > len(items) // 2
        else:                                                            # mostly rejections, at many different checks
            assert (want != 0).sum() > len(items) // 2 and len(set(want.tolist())) >= 12


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q", [(4, 1, 1), (5, 2, 2), (10, 3, 1)])
def test_k1_cpu_verifier_equals_the_reference_on_the_unfolded_corpus(zk, orc, log_n, log_b, q, hash_kind):
    """K = 1 is the degenerate case of the one verifier in transcript.hpp, so comparing it with zk_verify_check compares the code
    with itself.  This is its independent anchor: the plain-Python verifier of fold_ref.py at K = 1 over the corpus of the
    unfolded wire format (tests/verify_corpus.py, proofs from the oracle), strict and plain."""
    import verify_corpus
    lib = zk.load()
    items = verify_corpus.corpus(orc, log_n, log_b, q, hash_kind)
    for strict in (True, False):
        got = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, q, 0, 1, hash_kind, strict)
        want = np.array([fold_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, 0, 1)
                         for it in items], dtype=np.int32)
        bad = [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
        assert not bad, (strict, bad)
        assert want[0] == 0 and (want != 0).sum() > len(items) // 2
        if not strict:
            assert len(set(want.tolist())) >= 12


def test_eight_point_trace_proofs_are_valid(zk, orc):
    """log_n = 3 (groups of 2 + 1 at K = 2), which oracle.prove refuses: the proofs verify_fold_corpus assembles from the oracle's
    primitives are accepted by both CPU verifiers, strict and plain, and a flipped value is rejected by both with one number."""
    lib = zk.load()
    for log_b in (1, 2, 3):
        for K in (1, 2, 3):
            for hash_kind in (0, 1):
                proofs = verify_fold_corpus.ref_proofs(orc, 3, log_b, 2, 0, K, hash_kind)
                items = [verify_fold_corpus.Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(proofs)]
                d, s, last = proofs[0]
                items.append(verify_fold_corpus.Item("p0.last_byte", d[:-1] + bytes([d[-1] ^ 1]), s, last))
                for strict in (True, False):
                    got = verify_fold_corpus.cpu_checks(lib, items, 3, log_b, 2, 0, K, hash_kind, strict)
                    want = [fold_ref.verify(orc, it.data, it.state if strict else None, 3, log_b, it.public_last, hash_kind, 2, 0, K) for it in items]
                    assert got.tolist() == want and want[:2] == [0, 0] and want[2] != 0, (log_b, K, hash_kind, strict, got, want)


def test_null_handle(zk):
    lib = zk.load()
    assert lib.zk_verifier_set_fold(None, 2) == -1
    assert lib.zk_verifier_get_fold(None) == 0
