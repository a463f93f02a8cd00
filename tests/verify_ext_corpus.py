"""Tamper corpus for the batched verifier's tests of proofs over E = F_P[u] / (u^2 - 5) (tests/test_verify_ext_corpus.py,
tests/test_gpu_verify_ext.py): the counterpart of tests/verify_stop_corpus.py and tests/verify_cap_corpus.py for the wire format of
transcript.hpp with ext = 1.

The valid proofs come from tests/ext_ref.py, built without the library; ext_ref.regions gives the offsets, the two words of every value of E
as fields of their own (.c0 / .c1).  One variant per field as in verify_stop_corpus: of a path one node stands for the whole, of a cap one
entry -- the one the first query's path of the first proof lands in (entry 0 only where the cap has one entry or the query lands there), of
the never-opened last tree its last entry.  Every variant comes in the three kinds of verify_corpus (bit flip, plus P, swap with the other
proof); then the wrong public_last trio, a wrong state, an all-zero proof and two random-byte proofs (the malformed-layout path).

A shape with many queries has thousands of fields.  Its table is thinned per kind of field (the name with every number replaced by #, the
component kept): the first, the middle and the last field of each kind stay, so every kind stays for both components -- alpha#.c1,
beta#.c1, coef#.c1 / free_term.c1, q#.cp.c1, q#.g#.value#.c1 / q#.g#.slot#.c1 among them.  A verifier that compares only component 0
accepts what the CPU rejects on each of those."""
import re

import numpy as np

import ext_ref
import verify_fold_corpus
from verify_corpus import SEEDS, Item  # noqa: F401
from fold_ref import groups

# a1 of the two proofs of a shape (a0 = 1): verify_corpus.SEEDS serve every shape here -- each leaves a component-1 word w with
# w + P < 2^32 among the kept fields for both hashes (tests/test_verify_ext_corpus.py checks it).  A shape whose seeds would not is listed.
SHAPE_SEEDS = {}

# (log_n, log_b, q, g, K, coset, D, c): R = 2, the minimum; one full group with a 16-word leaf and a short last group; Horner on both
# planes, a cap and four 2-word leaves per group; eight non-adjacent (c0, c1) pairs and the ce = lg - 1 clamp on the small trees; K = 2
# coset leaves with 16 coefficients per plane; the reference's size
SHAPES = [(2, 1, 1, 0, 1, False, 0, 0), (4, 2, 2, 8, 3, True, 0, 0), (5, 2, 7, 0, 2, False, 2, 4), (6, 1, 2, 0, 3, False, 0, 8),
          (7, 2, 3, 8, 2, True, 4, 4), (10, 3, 1, 0, 1, True, 2, 0)]

KEPT_C1_KINDS = ("alpha#.c1", "beta#.c1", "coef#.c1", "free_term.c1", "q#.cp.c1", "q#.g#.value#.c1", "q#.g#.slot#.c1")
THIN_ABOVE = 50          # fields; thinned to three per kind, about 300 items

_PATH = re.compile(r"^q(\d+)\.(f|cp|g)(\d*)\.path(\d*)$")
_CAP = re.compile(r"^(f_root|root(\d+))\.e(\d+)$")


def kind_of(name):
    """The name with every number replaced by #, the component (.c0 / .c1) kept."""
    m = re.search(r"\.c([01])$", name)
    stem = name[:m.start()] if m else name
    return re.sub(r"\d+", "#", stem) + (m.group(0) if m else "")


def landed_entries(ref, log_n, log_b, K, coset, D, c):
    """{cap name: the entry the first query's first path into that tree lands in}; the last tree (D = 0), which nothing opens: its last."""
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    grp = groups(log_n - D, K)
    lg = dict(ext_ref.trees(log_n, log_b, K, coset, D))
    x = ref.raws[0] % (N - 2 * B)
    out = {"f_root": x >> (L - ext_ref.c_eff(c, L))}
    for j, (r0, steps) in enumerate(grp):
        tid = 1 + r0
        leaf = x % (1 << lg[tid])                             # value 0 of the group, or the group's one leaf
        out[f"root{j}"] = leaf >> (lg[tid] - ext_ref.c_eff(c, lg[tid]))
    if not D:
        tid = 1 + log_n
        out[f"root{len(grp)}"] = (1 << ext_ref.c_eff(c, lg[tid])) - 1
    return out


def fields(ref, log_n, log_b, q, g, K, coset, D, c):
    """(name, byte offset, size, kind) of the tampered fields; kind is "value" (u32), "digest" (32 bytes), "count" (u64).  `ref` (the
    first proof) says which entry of a cap stands for it."""
    entry = landed_entries(ref, log_n, log_b, K, coset, D, c)
    out = []
    for name, off, size in ext_ref.regions(log_n, log_b, q, g, K, coset, D, c):
        m, mc = _PATH.match(name), _CAP.match(name)
        if mc:
            if int(mc.group(3)) == entry[mc.group(1)]:
                out.append((name, off, 32, "digest"))
        elif m:
            plen = size // 32
            if plen:
                node = (int(m.group(1)) + int(m.group(3) or 0) + int(m.group(4) or 0)) % plen
                out.append((f"{name}.node{node}", off + 32 * node, 32, "digest"))
        elif name == "nonce" or ".count" in name:
            out.append((name, off, size, "count"))
        else:
            assert size == 4, name
            out.append((name, off, size, "value"))               # alphas, betas, free term / coefficients, raws, values, slots: one word each
    if len(out) > THIN_ABOVE:
        by_kind = {}
        for f in out:
            by_kind.setdefault(kind_of(f[0]), []).append(f)
        keep = set()
        for fs in by_kind.values():
            keep.update(fs[i][0] for i in {0, len(fs) // 2, len(fs) - 1})
        out = [f for f in out if f[0] in keep]
    return out


def ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """The two valid proofs of one shape as ext_ref builds them (.data, .state, .public_last, .raws, .c)."""
    seeds = SHAPE_SEEDS.get((log_n, log_b, q, g, K, bool(coset), D, c), SEEDS)
    return [ext_ref.proof(orc, log_n, log_b, q, hash_kind, K, bool(coset), D, c, g, a1) for a1 in seeds]


def ref_proofs(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """[(data, state, public_last)] of the two valid proofs."""
    return [(r.data, r.state, r.public_last) for r in ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)]


_corpora = {}


def corpus(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """The corpus of one shape, built once per session and shared (Items are immutable: bytes and ints)."""
    key = (log_n, log_b, q, g, K, bool(coset), D, c, hash_kind)
    if key not in _corpora:
        refs = ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)
        _corpora[key] = verify_fold_corpus.variants([(r.data, r.state, r.public_last) for r in refs],
                                                    fields(refs[0], log_n, log_b, q, g, K, coset, D, c))
    return _corpora[key]


def cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, c, hash_kind, strict):
    """zk_verify_ext's check number (ext_log = 1) for every item, as an int32 array."""
    import ctypes as C
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        n = C.c_int32(12345)
        rc = lib.zk_verify_ext(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last & 0xFFFFFFFF, hash_kind, q, g, K,
                               int(bool(coset)), D, c, 1, C.byref(n))
        assert rc == (0 if n.value == 0 else -6), (it.label, rc, n.value)
        out[i] = n.value
    return out
