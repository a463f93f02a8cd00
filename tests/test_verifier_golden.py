"""The CPU verifier against check numbers recorded before its K = 1 and folded halves became one (no GPU).

tests/golden/verifier_checks.json (tools/record_verifier_checks.py) holds, for every item of the tamper corpora at five shapes,
the strict and the plain check number the two separate verifiers gave.  On the K = 1 shapes every entry point that can express
the call -- zk_verify_fold with fold_log 1, zk_verify_grind with no nonce, zk_verify_check, and zk_verify_queries through accept /
reject and the number in its message -- must still give them; on the folded shapes zk_verify_fold must.  The file also carries
a SHA-256 of each corpus, so that a corpus that drifted is not mistaken for a verifier that did."""
import ctypes as C
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import record_verifier_checks as rec                       # noqa: E402

with open(rec.OUT) as _f:
    GOLDEN = json.load(_f)["shapes"]
KEYS = ("log_n", "log_b", "q", "g", "K", "hash")


def _id(s):
    return "-".join(f"{k}{s[k]}" for k in KEYS)


@pytest.fixture(scope="module")
def corpora(orc):
    return {tuple(key[k] for k in KEYS): items for key, items in rec.shapes(orc)}


def test_the_file_covers_the_shapes():
    want = [(n, b, q, 0, 1, h) for n, b, q in rec.K1_SHAPES for h in (0, 1)] + [s + (0,) for s in rec.FOLD_SHAPES]
    assert [tuple(s[k] for k in KEYS) for s in GOLDEN] == want
    assert 1000 < sum(len(s["rows"]) for s in GOLDEN) < 10000


@pytest.mark.parametrize("shape", GOLDEN, ids=_id)
def test_check_numbers_are_the_recorded_ones(zk, corpora, shape):
    lib = zk.load()
    log_n, log_b, q, g, K, hk = key = tuple(shape[k] for k in KEYS)
    items = corpora[key]
    assert rec.corpus_digest(items) == shape["sha256"], "the corpus itself changed: not a statement about the verifier"
    assert [it.label for it in items] == [r[0] for r in shape["rows"]]
    bad = []
    for it, (label, strict, plain) in zip(items, shape["rows"]):
        for state, want in ((it.state, strict), (None, plain)):
            want_rc = 0 if want == 0 else -6
            got = {}
            c = C.c_int32(12345)
            rc = lib.zk_verify_fold(it.data, len(it.data), state, log_n, log_b, it.public_last, hk, q, g, K, C.byref(c))
            got["zk_verify_fold"] = (rc, c.value)
            if K == 1:
                c = C.c_int32(12345)
                rc = lib.zk_verify_grind(it.data, len(it.data), state, log_n, log_b, it.public_last, hk, q, 0, C.byref(c))
                got["zk_verify_grind"] = (rc, c.value)
                c = C.c_int32(12345)
                rc = lib.zk_verify_check(it.data, len(it.data), state, log_n, log_b, it.public_last, hk, q, C.byref(c))
                got["zk_verify_check"] = (rc, c.value)
                rc = lib.zk_verify_queries(it.data, len(it.data), state, log_n, log_b, it.public_last, hk, q)
                m = re.search(r"at check (-?\d+)", lib.zk_last_error().decode()) if rc else None
                assert rc == 0 or m, lib.zk_last_error()
                got["zk_verify_queries"] = (rc, int(m.group(1)) if rc else 0)
            bad += [(label, state is not None, who, v, want) for who, v in got.items() if v != (want_rc, want)]
    assert not bad, bad[:20]
