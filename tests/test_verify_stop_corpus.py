"""The tamper corpus of proofs that stop FRI early (tests/verify_stop_corpus.py) without a GPU: its field table covers the wire
format with no gap in the header, both valid proofs of every shape pass zk_verify_stop and the plain-Python verifier of
tests/stop_ref.py, and the corpus holds the inputs the batched GPU verifier's exactness test needs -- rejected coefficients in plain
and in strict mode, raw coefficients >= P that plain mode accepts, the malformed-layout items and the wrong state.  These are
conditions on the inputs, checked before anything goes to a GPU."""
import struct

import numpy as np
import pytest

import stop_ref
import verify_stop_corpus
from verify_corpus import P

SHAPES = verify_stop_corpus.SHAPES


def test_field_table_covers_the_length():
    for log_n in range(2, 11):
        for K in (1, 2, 3):
            for coset in (False, True):
                for D in (1, 2, log_n - 1, 8):
                    if not stop_ref.admissible(log_n, 2, D):
                        continue
                    for g in (0, 8):
                        for q in (1, 3):
                            table = verify_stop_corpus.fields(log_n, 2, q, g, K, coset, D)
                            spans = sorted((off, off + size) for _, off, size, _ in table)
                            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (log_n, K, coset, D, g, q)   # no two fields overlap
                            assert spans[-1][1] <= stop_ref.proof_len(log_n, 2, q, g, K, coset, D)
                            names = [n for n, _, _, _ in table]
                            assert len(set(names)) == len(names)
                            # the header is covered byte for byte: no gap before query 0's openings
                            head = verify_stop_corpus.header_bytes(log_n, 2, q, g, K, D)
                            pos = 0
                            for lo, hi in spans:
                                if lo >= head:
                                    break
                                assert lo == pos, (log_n, K, coset, D, g, q, lo, pos)
                                pos = hi
                            assert pos == head
                            grp = stop_ref.groups(log_n - D, K)
                            G = len(grp)
                            per_q = (9 + sum((1 << s) + 2 for _, s in grp)) if coset else (12 + sum(3 * (1 << s) for _, s in grp))
                            assert len(table) == 5 + 2 * G - 1 + (1 << D) + (1 if g else 0) + q + q * per_q
                            assert not any(n == "free_term" or n == f"root{G}" for n in names)
                            assert sum(n.startswith("coef") for n in names) == 1 << D


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K,coset,D", SHAPES)
def test_the_corpus_is_worth_running(zk, orc, log_n, log_b, q, g, K, coset, D, hash_kind):
    lib = zk.load()
    items = verify_stop_corpus.corpus(orc, log_n, log_b, q, g, K, coset, D, hash_kind)
    labels = [it.label for it in items]
    G = len(stop_ref.groups(log_n - D, K))
    checks = {s: verify_stop_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, hash_kind, s) for s in (True, False)}
    valid = [i for i, lab in enumerate(labels) if lab.endswith(".valid")]
    assert len(valid) == 2
    for i in valid:                                           # both valid proofs: the library's CPU verifier and the plain-Python one
        it = items[i]
        assert len(it.data) == lib.zk_proof_data_len_stop(log_n, log_b, q, g, K, int(coset), D)
        for strict in (True, False):
            assert checks[strict][i] == 0
            assert stop_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K, coset, D) == 0
    coef = [i for i, lab in enumerate(labels) if ".coef" in lab]
    assert len(coef) >= 2 * (1 << D)                          # every coefficient of both proofs has at least its bit flip
    for strict in (True, False):
        want = checks[strict]
        print(f"shape {(log_n, log_b, q, g, K, coset, D)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
              f"{len(set(want.tolist()))} distinct check numbers")
        assert (want != 0).sum() > len(items) // 2            # mostly rejections
    # plain: a tampered coefficient fails the last group's comparison, which keeps its number
    assert -(100 + (G - 1)) in {int(checks[False][i]) for i in coef}
    # strict: it changes the channel state, so the first query challenge (k = 3 + G' + 1) or, with grinding, the nonce test fails
    strict_coef = {int(checks[True][i]) for i in coef}
    assert all(c == -1998 or c < -(1000 + 3 + G) for c in strict_coef), strict_coef
    assert (-1998 in strict_coef) if g else (-(1000 + 3 + G + 1) in strict_coef)
    if D >= 4:
        # a raw coefficient >= P with the same residue: reduced on reading, so plain mode accepts it; the replay hashes the raw bytes
        plus = [i for i in coef if labels[i].endswith(".plusP")]
        assert plus, "no coefficient c with c + P < 2^32: choose other seeds (verify_stop_corpus.SHAPE_SEEDS)"
        for i in plus:
            off = next(o for n, o, _, _ in verify_stop_corpus.fields(log_n, log_b, q, g, K, coset, D) if n == labels[i].split(".")[1])
            assert struct.unpack_from("<I", items[i].data, off)[0] >= P
            assert checks[False][i] == 0 and checks[True][i] != 0, (labels[i], checks[False][i], checks[True][i])
    # the malformed-layout path of the batched verifier and the wrong state
    assert {"zeros", "random0", "random1", "p0.state", "p1.state"} <= set(labels)
    assert checks[True][labels.index("p0.state")] == -1999 and checks[False][labels.index("p0.state")] == 0
    for lab in ("zeros", "random0", "random1"):
        assert checks[False][labels.index(lab)] != 0
