"""Proofs with several faults, for the ordering claim of the batched GPU verifier (tests/test_verify_multi_corpus.py,
tests/test_gpu_verify_multi.py): every element of checks_out is the number at which the CPU verifier stops FIRST, whatever else is
wrong with the proof.  The single-fault corpora (verify_corpus, verify_fold_corpus, verify_coset_corpus) change one field each, so
an order key that is position-major, a keys constant that is too small or a wrong position of one path slot leaves them green.

One generator serves the three wire formats: "plain" (K = 1, proofs from the oracle), "fold" (K = 2, 3, tests/fold_ref.py) and
"coset" (K = 1, 2, 3, tests/coset_ref.py).  From the field table of the format it derives one fault class per check the verifier
can fail at -- per query: cp0, each f / cp path, each group's fold comparison, each group's path (one-value leaves: path t = 0 and
the last path t >= 1), each path count; global: the f root, the cp root, one alpha, each beta, each group root, the free term, the
nonce, one query raw, public_last and the state.  The representative of a class is the "flip" variant of the single-fault corpora
(one bit, the same bit rule).  Every class carries its query and its position in the verifier's order (the position of the device's
order key: verify.hip).  The corpus of a shape is the valid proofs, every single fault on both proofs, every unordered pair of
classes and a seeded sample of triples, all faults of an item applied to the same valid proof (pairs and triples alternate between
the two proofs of the shape).
"""
import ctypes as C
import itertools

import numpy as np

import coset_ref
import fold_ref
import verify_corpus
import verify_coset_corpus
import verify_fold_corpus
from verify_corpus import Item

# (format, log_n, log_b, q, grind bits, K): the smallest shapes at which every key position exists and the three queries are far
# enough apart for a query-major and a position-major order to differ.  Groups: 5 rounds; 2+2+1; 3+1; one of 3; 2+2+1; 3+2; 1+1+1+1.
# In the fourth the last group is full, so its last path has the last position of the folded scheme, 4 + 9G: the other folded
# shapes end on a short group and leave the top of the key range unused.
SHAPES = [("plain", 5, 2, 3, 0, 1), ("fold", 5, 2, 3, 8, 2), ("fold", 4, 1, 3, 0, 3), ("fold", 3, 2, 3, 0, 3),
          ("coset", 5, 2, 3, 8, 2), ("coset", 5, 2, 3, 0, 3), ("coset", 4, 1, 3, 0, 1)]
FORMATS = ("plain", "fold", "coset")

PAIR_LIMIT = 3000      # a shape with more pairs than this keeps every pair that involves a per-query class of query 0 or 2 ...
REST_SAMPLE = 300      # ... and this many of the others (the pairs inside query 1, query 1 with a global class, two global classes)
TRIPLES = 200
SEED = 20240611


class Fault:
    """One fault class on one valid proof.  query: 0..q-1, or None for a global field.  pos: the position of the check it fails in
    the verifier's order within a query (the device's order key is query * keys + pos), None for counts and global fields.
    kind: "algebra" (cp0, a fold comparison), "paths", "count", "global".  where: (offset, size) in the proof bytes, or
    "public_last" / "state"."""

    def __init__(self, name, query, pos, kind, where):
        self.name, self.query, self.pos, self.kind, self.where = name, query, pos, kind, where


class MultiItem(Item):
    def __init__(self, label, data, state, public_last, proof, faults):
        super().__init__(label, data, state, public_last)
        self.proof, self.faults = proof, tuple(faults)       # index of the valid proof; indices into Corpus.classes[proof]


class Corpus:
    """items: every proof to check.  classes[p]: the Faults on valid proof p (the same names and order for every p).
    valid[p], single[(p, a)]: item indices.  pairs: (item index, p, a, b); triples: (item index, p, a, b, c)."""

    def __init__(self):
        self.items, self.classes, self.valid, self.single, self.pairs, self.triples = [], [], [], {}, [], []


def field_table(fmt, log_n, log_b, q, g, K):
    if fmt == "plain":
        assert g == 0 and K == 1
        return verify_corpus.fields(log_n, log_b, q)
    return (verify_fold_corpus if fmt == "fold" else verify_coset_corpus).fields(log_n, log_b, q, g, K)


def valid_proofs(orc, fmt, log_n, log_b, q, g, K, hash_kind):
    if fmt == "plain":
        return verify_corpus.oracle_proofs(orc, log_n, log_b, q, hash_kind)
    return (verify_fold_corpus if fmt == "fold" else verify_coset_corpus).ref_proofs(orc, log_n, log_b, q, g, K, hash_kind)


def fault_classes(fmt, log_n, log_b, q, g, K, data):
    """The fault classes of one valid proof (data: its bytes; the coset format reads the query raws from it to tell value 0 of a
    group from the other slots)."""
    table = field_table(fmt, log_n, log_b, q, g, K)
    where = {name: (off, size) for name, off, size, _ in table}
    L = log_n + log_b
    grp = fold_ref.groups(log_n, K)
    G = len(grp)

    def starting(prefix):                                    # the one node field of a path: its level is part of the name
        hits = [n for n in where if n.startswith(prefix)]
        assert len(hits) == 1, (prefix, hits)
        return hits[0]

    out = []

    def add(name, query, pos, kind, field=None):
        out.append(Fault(name, query, pos, kind, where[field or name] if (field or name) in where else (field or name)))

    nf = 3 if fmt == "coset" else 4
    for k in range(q):
        add(f"q{k}.cp0", k, 0, "algebra", f"q{k}.f0.value")                       # f(x) changed: cp0 fails before the f(x) path
        for i in range(nf):
            add(starting(f"q{k}.f{i}.node"), k, 1 + i, "paths")
        if fmt == "plain":
            for i in range(G):                                                      # -x of layer i: its fold, then its path
                add(f"q{k}.fold{i}", k, 5 + i, "algebra", f"q{k}.layer{i}.nx")
            for i in range(G):
                add(starting(f"q{k}.layer{i}.x_node"), k, 5 + G + 2 * i, "paths")
                add(starting(f"q{k}.layer{i}.nx_node"), k, 5 + G + 2 * i + 1, "paths")
            counts = [f"q{k}.f{i}.count" for i in range(4)] + [f"q{k}.layer{i}.{w}_count" for i in range(G) for w in ("x", "nx")]
        elif fmt == "fold":
            for j in range(G):                                                      # a value that is not value 0: this group's fold
                add(f"q{k}.fold{j}", k, 5 + j, "algebra", f"q{k}.group{j}.v1")
            for j, (_, steps) in enumerate(grp):
                last = (1 << steps) - 1
                add(starting(f"q{k}.group{j}.p0.node"), k, 5 + G + 8 * j, "paths")
                add(starting(f"q{k}.group{j}.p{last}.node"), k, 5 + G + 8 * j + last, "paths")
            counts = [f"q{k}.f{i}.count" for i in range(4)] + [f"q{k}.group{j}.p{t}.count" for j, (_, s) in enumerate(grp) for t in range(1 << s)]
        else:
            raw = int.from_bytes(data[where[f"query_raw{k}"][0]:][:4], "little")
            tp = raw % ((1 << L) - 2 * (1 << log_b))
            for j, (r0, steps) in enumerate(grp):                                  # value 1 sits in slot (rot + 1) % s
                rot = (tp & ((1 << (L - r0)) - 1)) >> (L - r0 - steps)
                add(f"q{k}.fold{j}", k, 4 + j, "algebra", f"q{k}.group{j}.slot{(rot + 1) % (1 << steps)}")
            for j in range(G):
                add(starting(f"q{k}.group{j}.node"), k, 4 + G + j, "paths")
            counts = [f"q{k}.f{i}.count" for i in range(3)] + [f"q{k}.group{j}.count" for j in range(G)]
        for name in counts:
            add(name, k, None, "count")
    roots = "layer_root" if fmt == "plain" else "group_root"
    for name in ["f_root", "cp_root", "alpha1"] + [f"beta{j}" for j in range(G)] + [f"{roots}{j}" for j in range(G)] + ["free_term"] \
            + (["nonce"] if g else []) + [f"query_raw{q // 2}", "public_last", "state"]:
        add(name, None, None, "global")
    assert len({f.name for f in out}) == len(out)
    return out


def _flip(data, off, size, proof):
    """The "flip" variant of the single-fault corpora: one bit of the field, chosen by its offset and the proof's index."""
    bit = (off * 7 + proof) % (8 * size)
    out = bytearray(data)
    out[off + bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


def apply(proof, valid, faults):
    """The valid proof (data, state, public_last) with every fault of `faults` applied."""
    data, state, last = valid
    for f in faults:
        if f.where == "public_last":
            last = last + 1
        elif f.where == "state":
            state = state[:5] + bytes([state[5] ^ 0x10]) + state[6:]   # the wrong state of the single-fault corpora
        else:
            data = _flip(data, f.where[0], f.where[1], proof)
    return data, state, last


def pair_selection(classes):
    """The (a, b) index pairs of a shape: all of them, or above PAIR_LIMIT every pair that involves a per-query class of query 0
    or 2 and a seeded sample of the others."""
    every = list(itertools.combinations(range(len(classes)), 2))
    if len(every) <= PAIR_LIMIT:
        return every
    keep = [ab for ab in every if any(classes[i].query in (0, 2) for i in ab)]
    rest = [ab for ab in every if not any(classes[i].query in (0, 2) for i in ab)]
    rng = np.random.default_rng(SEED)
    return keep + [rest[i] for i in sorted(rng.choice(len(rest), min(REST_SAMPLE, len(rest)), replace=False))]


_corpora = {}


def corpus(orc, fmt, log_n, log_b, q, g, K, hash_kind):
    """The multi-fault corpus of one shape, built once per session and shared (nothing in it is changed by a test)."""
    key = (fmt, log_n, log_b, q, g, K, hash_kind)
    if key in _corpora:
        return _corpora[key]
    proofs = valid_proofs(orc, fmt, log_n, log_b, q, g, K, hash_kind)
    c = Corpus()
    c.classes = [fault_classes(fmt, log_n, log_b, q, g, K, d) for d, _, _ in proofs]
    assert all([f.name for f in cl] == [f.name for f in c.classes[0]] for cl in c.classes)

    def emit(p, idx):
        faults = [c.classes[p][i] for i in idx]
        label = f"p{p}|" + "+".join(f.name for f in faults) if idx else f"p{p}.valid"
        c.items.append(MultiItem(label, *apply(p, proofs[p], faults), p, idx))
        return len(c.items) - 1

    for p in range(len(proofs)):
        c.valid.append(emit(p, ()))
        for a in range(len(c.classes[p])):
            c.single[(p, a)] = emit(p, (a,))
    for n, (a, b) in enumerate(pair_selection(c.classes[0])):
        p = n % len(proofs)
        c.pairs.append((emit(p, (a, b)), p, a, b))
    rng = np.random.default_rng(SEED + 1)
    seen = set()
    while len(c.triples) < TRIPLES:
        abc = tuple(sorted(int(i) for i in rng.choice(len(c.classes[0]), 3, replace=False)))
        if abc in seen:
            continue
        seen.add(abc)
        p = len(c.triples) % len(proofs)
        c.triples.append((emit(p, abc), p) + abc)
    _corpora[key] = c
    return c


def cpu_checks(lib, items, fmt, log_n, log_b, q, g, K, hash_kind, strict):
    """The C verifier's check number for every item as an int32 array: zk_verify_check, zk_verify_fold or zk_verify_coset."""
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        c = C.c_int32(12345)
        state = it.state if strict else None
        if fmt == "plain":
            rc = lib.zk_verify_check(it.data, len(it.data), state, log_n, log_b, it.public_last, hash_kind, q, C.byref(c))
        else:
            fn = lib.zk_verify_fold if fmt == "fold" else lib.zk_verify_coset
            rc = fn(it.data, len(it.data), state, log_n, log_b, it.public_last, hash_kind, q, g, K, C.byref(c))
        assert rc == (0 if c.value == 0 else -6), (it.label, rc, c.value)
        out[i] = c.value
    return out


_cpu = {}


def cpu_numbers(lib, orc, shape, hash_kind, strict):
    """cpu_checks over the whole corpus of a shape, computed once per session."""
    key = (shape, hash_kind, strict)
    if key not in _cpu:
        _cpu[key] = cpu_checks(lib, corpus(orc, *shape, hash_kind).items, *shape, hash_kind, strict)
        _cpu[key].setflags(write=False)
    return _cpu[key]


def ref_checks(orc, items, fmt, log_n, log_b, q, g, K, hash_kind, strict):
    """The plain-Python verifier's number for every item (fold_ref.verify; coset_ref.verify for coset leaves)."""
    fn = coset_ref.verify if fmt == "coset" else fold_ref.verify
    return np.array([fn(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K) for it in items],
                    dtype=np.int32)


def transcript_state(fmt, data, log_n, log_b, q, g, K):
    """The state the Fiat-Shamir channel ends in over these proof bytes (the commit schedule of fold_ref.replay / coset_ref.replay
    without the challenge tests): with it a proof tampered after the last challenge passes the strict replay, so strict mode
    reaches the checks of verify_proof."""
    L = log_n + log_b
    grp = fold_ref.groups(log_n, K)
    sizes = [32, 4, 4, 4, 32] + [4, 32] * len(grp) + [4] + ([8] if g else []) + [4] * q
    for _ in range(q):
        sizes += [12 + 32 * L] * (3 if fmt == "coset" else 4)
        for r0, steps in grp:
            sizes.append(4 * (1 << steps) + 8 + 32 * (L - r0 - steps) if fmt == "coset" else (1 << steps) * (12 + 32 * (L - r0)))
    assert sum(sizes) == len(data)
    ch, pos = fold_ref._Channel(), 0
    for n in sizes:
        ch.commit(data[pos:pos + n])
        pos += n
    return ch.state


def path_regions(fmt, log_n, log_b, q, g, K, data):
    """(offset of the first digest, digests) of every path of a valid proof: each u64 count of the field table and its value."""
    return [(off + 8, int.from_bytes(data[off:off + 8], "little")) for name, off, _, kind in field_table(fmt, log_n, log_b, q, g, K)
            if kind == "count" and name != "nonce"]
