"""Tamper corpus for the verifier tests of proofs with coset leaves (tests/test_verify_coset_corpus.py,
tests/test_gpu_verify_coset.py): the counterpart of tests/verify_fold_corpus.py for the wire format of transcript.hpp with
coset = true (proof_data_len / verify_proof / verify_transcript).

The valid proofs come from tests/coset_ref.py, built without the library.  For each there is one variant per field: the f root,
each alpha, the cp root, each group's beta and output root, the free term, the nonce, each query raw, and per query the three f
values with their counts and one node each, then per group every one of its s slots, the count and one node of its one path.
Every variant comes in the three kinds of verify_corpus (bit flip, plus P, swap with the other proof); then the wrong public_last
trio, a wrong state, an all-zero proof and two random-byte proofs (the malformed-layout path of the batched verifier).
"""
import numpy as np

import coset_ref
import fold_ref
import verify_fold_corpus
from verify_corpus import SEEDS, Item  # noqa: F401  (Item: what the tests build their own batches from)

# a1 of the two proofs of a shape (a0 = 1): verify_corpus.SEEDS, except where those leave a slot rotation of the one full group
# unvisited -- with these two, the 14 query indices of the K = 3, q = 7 shape put value 0 of group 0 in every slot 0..7, for both
# hashes (tests/test_verify_coset_corpus.py checks it)
SHAPE_SEEDS = {(5, 2, 7, 8, 3): (3141592, 3141602)}


def fields(log_n, log_b, q, g, K):
    """(name, byte offset, size, kind) of every field; kind is "value" (u32), "digest" (32 bytes), "count" (u64)."""
    L = log_n + log_b
    grp = fold_ref.groups(log_n, K)
    G = len(grp)
    out = [("f_root", 0, 32, "digest")]
    out += [(f"alpha{i}", 32 + 4 * i, 4, "value") for i in range(3)]
    out.append(("cp_root", 44, 32, "digest"))
    for j in range(G):
        out.append((f"beta{j}", 76 + 36 * j, 4, "value"))
        out.append((f"group_root{j}", 80 + 36 * j, 32, "digest"))
    out.append(("free_term", 76 + 36 * G, 4, "value"))
    qraw = 80 + 36 * G
    if g:
        out.append(("nonce", qraw, 8, "count"))
        qraw += 8
    out += [(f"query_raw{k}", qraw + 4 * k, 4, "value") for k in range(q)]
    pos = qraw + 4 * q
    for k in range(q):
        for i in range(3):                                   # f(x), f(gx), f(g^2 x)
            node = (k + i) % L
            out += [(f"q{k}.f{i}.value", pos, 4, "value"), (f"q{k}.f{i}.count", pos + 4, 8, "count"),
                    (f"q{k}.f{i}.node{node}", pos + 12 + 32 * node, 32, "digest")]
            pos += 12 + 32 * L
        for j, (r0, steps) in enumerate(grp):
            s, plen = 1 << steps, L - r0 - steps
            out += [(f"q{k}.group{j}.slot{u}", pos + 4 * u, 4, "value") for u in range(s)]
            pos += 4 * s
            node = (k + j) % plen
            out += [(f"q{k}.group{j}.count", pos, 8, "count"), (f"q{k}.group{j}.node{node}", pos + 8 + 32 * node, 32, "digest")]
            pos += 8 + 32 * plen
    assert pos == coset_ref.proof_len(log_n, log_b, q, g, K)
    return out


def ref_objects(orc, log_n, log_b, q, g, K, hash_kind):
    """The two valid coset-leaf proofs of one size as coset_ref builds them (.data, .state, .public_last, .raws)."""
    if log_n == 3:                                           # one proxy per oracle, shared with the folded corpus: coset_ref caches by identity
        orc = verify_fold_corpus._n8.setdefault(id(orc), verify_fold_corpus._OracleWithN8(orc))
    out = []
    for a1 in SHAPE_SEEDS.get((log_n, log_b, q, g, K), SEEDS):
        r = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, bits=g, a1=a1)
        assert len(r.data) == coset_ref.proof_len(log_n, log_b, q, g, K)
        out.append(r)
    return out


def ref_proofs(orc, log_n, log_b, q, g, K, hash_kind):
    """[(data, state, public_last)] of the two valid proofs."""
    return [(r.data, r.state, r.public_last) for r in ref_objects(orc, log_n, log_b, q, g, K, hash_kind)]


_corpora = {}


def corpus(orc, log_n, log_b, q, g, K, hash_kind):
    """The corpus of one shape, built once per session and shared (Items are immutable: bytes and ints)."""
    key = (log_n, log_b, q, g, K, hash_kind)
    if key not in _corpora:
        _corpora[key] = verify_fold_corpus.variants(ref_proofs(orc, log_n, log_b, q, g, K, hash_kind), fields(log_n, log_b, q, g, K))
    return _corpora[key]


def cpu_checks(lib, items, log_n, log_b, q, g, K, hash_kind, strict, fn="zk_verify_coset"):
    """zk_verify_coset's check number for every item, as an int32 array (fn: another verifier of the same signature)."""
    import ctypes as C
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        c = C.c_int32(12345)
        rc = getattr(lib, fn)(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K, C.byref(c))
        assert rc == (0 if c.value == 0 else -6), (it.label, rc, c.value)
        out[i] = c.value
    return out
