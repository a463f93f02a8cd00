"""Tamper corpus for the batched verifier's tests of proofs with Merkle caps (tests/test_gpu_verify_cap.py): the counterpart of
tests/verify_stop_corpus.py for the wire format of transcript.hpp with cap = c > 0.

The valid proofs come from tests/cap_ref.py, built without the library; cap_ref.regions gives the offsets.  One variant per field as in
verify_stop_corpus.  Of a cap (up to 256 entries) the first and the last entry stand in, with up to two entries some path of the first
proof lands in and up to two none does: the first kind fails a path check, the second passes every path check and is caught by the
transcript replay alone.  Every variant comes in the three kinds of verify_corpus (bit flip, plus P, swap with the other proof); then
the wrong public_last trio, a wrong state, an all-zero proof and two random-byte proofs (the malformed-layout path)."""
import re

import numpy as np

import cap_ref
import verify_fold_corpus
from verify_corpus import SEEDS, Item  # noqa: F401

_PATH = re.compile(r"^q(\d+)\.(f|g)(\d+)\.path(\d*)$")
_CAP = re.compile(r"^(f_root|root(\d+))\.e(\d+)$")

# (log_n, log_b, q, g, K, coset, D, c): the smallest shape with every tree clamped; (6, 3) folded by 8 with coset leaves and an early
# stop, and unfolded to a constant; (10, 3) with c at, and below, the size of a SHA-256 hand-over
SHAPES = [(4, 1, 2, 0, 1, False, 0, 3), (4, 1, 1, 4, 2, True, 1, 8), (6, 3, 3, 4, 3, True, 2, 4), (6, 3, 2, 0, 1, False, 0, 2),
          (10, 3, 3, 0, 1, False, 0, 8), (10, 3, 2, 0, 3, True, 4, 4)]


def ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    return [cap_ref.proof(orc, log_n, log_b, q, hash_kind, K, bool(coset), D, c, g, a1) for a1 in SEEDS]


def ref_proofs(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """[(data, state, public_last)] of the two valid proofs."""
    return [(r.data, r.state, r.public_last) for r in ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)]


def fields(ref, log_n, log_b, q, g, K, coset, D, c):
    """(name, byte offset, size, kind) of the tampered fields; `ref` (the first proof) says which cap entries a path lands in."""
    tree_ids = sorted(t for t in ref.c.trees if t >= 1)
    out, taken = [], {}
    regs = cap_ref.regions(log_n, log_b, q, g, K, coset, D, c)
    last_entry = {}
    for name, _, _ in regs:
        m = _CAP.match(name)
        if m:
            last_entry[m.group(1)] = int(m.group(3))
    for name, off, size in regs:
        m = _PATH.match(name)
        mc = _CAP.match(name)
        if mc:
            tid = 0 if mc.group(1) == "f_root" else tree_ids[int(mc.group(2))]
            e = int(mc.group(3))
            landed = e in ref.landed[tid]
            n = taken.setdefault((mc.group(1), landed), 0)
            if e in (0, last_entry[mc.group(1)]) or n < 2:
                taken[(mc.group(1), landed)] = n + 1
                out.append((name + (".landed" if landed else ".free"), off, 32, "digest"))
        elif m:
            plen = size // 32
            node = (int(m.group(1)) + int(m.group(3)) + int(m.group(4) or 0)) % plen
            out.append((f"{name}.node{node}", off + 32 * node, 32, "digest"))
        elif name == "nonce" or ".count" in name:
            out.append((name, off, size, "count"))
        else:
            assert size == 4, name
            out.append((name, off, size, "value"))               # alphas, betas, free term / coefficients, raws, values, slots
    return out


_corpora = {}


def corpus(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind):
    """The corpus of one shape, built once per session and shared."""
    key = (log_n, log_b, q, g, K, bool(coset), D, c, hash_kind)
    if key not in _corpora:
        refs = ref_objects(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)
        _corpora[key] = verify_fold_corpus.variants([(r.data, r.state, r.public_last) for r in refs],
                                                    fields(refs[0], log_n, log_b, q, g, K, coset, D, c))
    return _corpora[key]


def cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, c, hash_kind, strict):
    """zk_verify_cap's check number for every item, as an int32 array."""
    import ctypes as C
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        n = C.c_int32(12345)
        rc = lib.zk_verify_cap(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last & 0xFFFFFFFF, hash_kind, q, g, K,
                               int(bool(coset)), D, c, C.byref(n))
        assert rc == (0 if n.value == 0 else -6), (it.label, rc, n.value)
        out[i] = n.value
    return out
