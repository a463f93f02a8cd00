"""Tamper corpus for the verifier tests of proofs that stop FRI early (tests/test_verify_stop_corpus.py,
tests/test_gpu_verify_stop.py): the counterpart of tests/verify_coset_corpus.py for the wire format of transcript.hpp with
stop = D > 0 (proof_data_len / verify_proof / verify_transcript), with one-value or coset leaves.

The valid proofs come from tests/stop_ref.py, built without the library; stop_ref.regions gives the offsets.  For each proof there is
one variant per field: the f root, each alpha, the cp root, each group's beta and -- for every group but the last, whose output has no
tree -- its output root, each of the 2^D coefficients (there is no free term), the nonce, each query raw, and per query the f (and cp)
values with their counts and one node each, then per group every opened value or slot and, for each of its paths, the count and one
node.  Every variant comes in the three kinds of verify_corpus (bit flip, plus P, swap with the other proof); then the wrong
public_last trio, a wrong state, an all-zero proof and two random-byte proofs (the malformed-layout path of the batched verifier).
"""
import re

import numpy as np

import stop_ref
import verify_fold_corpus
from verify_corpus import SEEDS, Item  # noqa: F401  (Item: what the tests build their own batches from)

# a1 of the two proofs of a shape (a0 = 1): verify_corpus.SEEDS serve every shape here -- in the D = 4 and D = 8 shapes they leave a
# coefficient c with c + P < 2^32 for both hashes (a third of all residues are; tests/test_verify_stop_corpus.py checks that the
# variant exists).  A shape whose seeds would not is listed here.
SHAPE_SEEDS = {}

# (log_n, log_b, q, g, K, coset, D): the smallest (R' = 1, one group, two coefficients, no group root in the header); one full group
# of eight slots with the nonce after the coefficients and seven queries; R' = 5 = 3 + 2 with one-value leaves; R' = 3 = 2 + 1; the
# largest D (256 coefficients) through the unfolded kernel; K = 1 coset leaves at the reference's size
SHAPES = [(2, 1, 1, 0, 1, False, 1), (5, 2, 7, 8, 3, True, 2), (6, 1, 2, 0, 3, False, 1), (7, 2, 3, 0, 2, True, 4),
          (9, 1, 1, 0, 1, False, 8), (10, 3, 2, 0, 1, True, 4)]

_PATH = re.compile(r"^q(\d+)\.(f|g)(\d+)\.path(\d*)$")


def fields(log_n, log_b, q, g, K, coset, D):
    """(name, byte offset, size, kind) of every field; kind is "value" (u32), "digest" (32 bytes), "count" (u64).  Of a path, one
    node (chosen by query, group and path number) stands for the whole."""
    out = []
    for name, off, size in stop_ref.regions(log_n, log_b, q, g, K, coset, D):
        m = _PATH.match(name)
        if m:
            plen = size // 32
            node = (int(m.group(1)) + int(m.group(3)) + int(m.group(4) or 0)) % plen
            out.append((f"{name}.node{node}", off + 32 * node, 32, "digest"))
        elif name == "nonce" or ".count" in name:
            out.append((name, off, size, "count"))
        elif size == 32:
            out.append((name, off, size, "digest"))              # f_root, root0 (cp), root1 .. root{G' - 1}
        else:
            assert size == 4, name
            out.append((name, off, size, "value"))               # alphas, betas, coefficients, raws, values, slots
    return out


def header_bytes(log_n, log_b, q, g, K, D):
    """Where query 0's openings start: 76 bytes, G' betas and G' - 1 roots, 2^D coefficients, the nonce, q raws."""
    G = len(stop_ref.groups(log_n - D, K))
    return 76 + 36 * (G - 1) + 4 + 4 * (1 << D) + (8 if g else 0) + 4 * q


def ref_objects(orc, log_n, log_b, q, g, K, coset, D, hash_kind):
    """The two valid stopped proofs of one shape as stop_ref builds them (.data, .state, .public_last, .raws, .coef)."""
    if log_n == 3:                                           # one proxy per oracle, shared with the folded corpus: stop_ref caches by identity
        orc = verify_fold_corpus._n8.setdefault(id(orc), verify_fold_corpus._OracleWithN8(orc))
    out = []
    for a1 in SHAPE_SEEDS.get((log_n, log_b, q, g, K, bool(coset), D), SEEDS):
        r = stop_ref.stop_proof(orc, log_n, log_b, q, hash_kind, K, bool(coset), D, bits=g, a1=a1)
        assert len(r.data) == stop_ref.proof_len(log_n, log_b, q, g, K, coset, D)
        out.append(r)
    return out


def ref_proofs(orc, log_n, log_b, q, g, K, coset, D, hash_kind):
    """[(data, state, public_last)] of the two valid proofs."""
    return [(r.data, r.state, r.public_last) for r in ref_objects(orc, log_n, log_b, q, g, K, coset, D, hash_kind)]


_corpora = {}


def corpus(orc, log_n, log_b, q, g, K, coset, D, hash_kind):
    """The corpus of one shape, built once per session and shared (Items are immutable: bytes and ints)."""
    key = (log_n, log_b, q, g, K, bool(coset), D, hash_kind)
    if key not in _corpora:
        _corpora[key] = verify_fold_corpus.variants(ref_proofs(orc, log_n, log_b, q, g, K, coset, D, hash_kind),
                                                    fields(log_n, log_b, q, g, K, coset, D))
    return _corpora[key]


def cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, hash_kind, strict):
    """zk_verify_stop's check number for every item, as an int32 array."""
    import ctypes as C
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        c = C.c_int32(12345)
        rc = lib.zk_verify_stop(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K,
                                int(bool(coset)), D, C.byref(c))
        assert rc == (0 if c.value == 0 else -6), (it.label, rc, c.value)
        out[i] = c.value
    return out
