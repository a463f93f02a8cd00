"""Tamper corpus for the verifier tests of folded proofs (tests/test_verify_fold_corpus.py, tests/test_gpu_verify_fold.py): the
counterpart of tests/verify_corpus.py for the wire format with a FRI folding factor 2^K (transcript.hpp: proof_data_len /
verify_proof with fold > 1).

The valid proofs come from tests/fold_ref.py, built without the library.  For each there is one variant per field: the f
root, each alpha, the cp root, each group's beta and output root, the free term, the nonce, each query raw, and per query the
four values with their counts and one node each, then per group every one of the s opened values and, for each of its s paths,
the count and one node.  Every variant comes in the three kinds of verify_corpus (bit flip, plus P, swap with the other proof);
then the wrong public_last trio, a wrong state, an all-zero proof and two random-byte proofs (the malformed-layout path of the
batched verifier).
"""
import numpy as np

import fold_ref
from verify_corpus import Item, P, SEEDS, _plus_p


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
        for i in range(4):                                   # f(x), f(gx), f(g^2 x), cp(x)
            node = (k + i) % L
            out += [(f"q{k}.f{i}.value", pos, 4, "value"), (f"q{k}.f{i}.count", pos + 4, 8, "count"),
                    (f"q{k}.f{i}.node{node}", pos + 12 + 32 * node, 32, "digest")]
            pos += 12 + 32 * L
        for j, (r0, steps) in enumerate(grp):
            s, plen = 1 << steps, L - r0
            out += [(f"q{k}.group{j}.v{t}", pos + 4 * t, 4, "value") for t in range(s)]
            pos += 4 * s
            for t in range(s):
                node = (k + j + t) % plen
                out += [(f"q{k}.group{j}.p{t}.count", pos, 8, "count"), (f"q{k}.group{j}.p{t}.node{node}", pos + 8 + 32 * node, 32, "digest")]
                pos += 8 + 32 * plen
    assert pos == fold_ref.proof_len(log_n, log_b, q, g, K)
    return out


def variants(proofs, table, rng_seed=0):
    """proofs: [(data, state, public_last)] of one size (at least two); table: fields(...).  The valid proofs and every variant."""
    out = []
    for i, (data, state, last) in enumerate(proofs):
        other = proofs[(i + 1) % len(proofs)][0]
        out.append(Item(f"p{i}.valid", data, state, last))
        for name, off, size, kind in table:
            field = data[off:off + size]
            bit = (off * 7 + i) % (8 * size)
            flipped = bytearray(field)
            flipped[bit // 8] ^= 1 << (bit % 8)
            for how, new in (("flip", bytes(flipped)), ("plusP", _plus_p(field, kind)), ("swap", other[off:off + size])):
                if new is None or new == field:
                    continue
                out.append(Item(f"p{i}.{name}.{how}", data[:off] + new + data[off + size:], state, last))
        out.append(Item(f"p{i}.public_last+1", data, state, last + 1))
        out.append(Item(f"p{i}.public_last+P", data, state, last + P))
        out.append(Item(f"p{i}.public_last^msb", data, state, last ^ 0x80000000))
        bad_state = bytearray(state)
        bad_state[5] ^= 0x10
        out.append(Item(f"p{i}.state", data, bytes(bad_state), last))
    rng = np.random.default_rng(rng_seed)
    n = len(proofs[0][0])
    out.append(Item("zeros", bytes(n), bytes(32), 0))
    for r in range(2):
        out.append(Item(f"random{r}", rng.integers(0, 256, n, dtype=np.uint8).tobytes(), rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
                        int(rng.integers(0, 2**32))))
    return out


class _ProveResult:
    pass


class _OracleWithN8:
    """The oracle with prove() at log_n = 3.  oracle.prove refuses n = 8 (g^4 = -1 makes the leading terms of f(gx)^2 + f(x)^2
    cancel, so the degree asserts of the reference's prover fail), but a verifier only wants cp to have degree < n: what fold_ref
    reads from prove()'s result -- f, public_last, and the first 76 transcript bytes and cp it cross-checks -- is assembled here
    from the oracle's own primitives.  Both CPU verifiers accept the proofs (tests/test_verify_fold_corpus.py)."""

    def __init__(self, orc):
        self._orc = orc

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def prove(self, log_n, log_b, a0, a1, want_vectors=True):
        if log_n != 3:
            return self._orc.prove(log_n, log_b, a0, a1, want_vectors=want_vectors)
        trace = self._orc.trace_fibsq((1 << log_n) - 1, a0, a1)
        r = _ProveResult()
        r.rc, r.public_last, r.f_eval = 0, int(trace[-1]), self._orc.lde(trace, log_n, log_b)
        ch = fold_ref._Channel()
        ch.commit(bytes(self._orc.merkle_build(r.f_eval)[0]))
        alphas = [ch.get_u32() for _ in range(3)]
        r.cp_layers = [self._orc.compose(r.f_eval, log_n, log_b, alphas, r.public_last)]
        ch.commit(bytes(self._orc.merkle_build(r.cp_layers[0])[0]))
        r.proof = bytes(ch.data)
        return r


_n8 = {}


def ref_proofs(orc, log_n, log_b, q, g, K, hash_kind):
    """Two valid folded proofs of one size from fold_ref: [(data, state, public_last)]."""
    if log_n == 3:
        orc = _n8.setdefault(id(orc), _OracleWithN8(orc))     # one proxy per oracle: fold_ref caches by its identity
    out = []
    for a1 in SEEDS:
        r = fold_ref.fold_proof(orc, log_n, log_b, q, hash_kind, K, bits=g, a1=a1)
        assert len(r.data) == fold_ref.proof_len(log_n, log_b, q, g, K)
        out.append((r.data, r.state, r.public_last))
    return out


_corpora = {}


def corpus(orc, log_n, log_b, q, g, K, hash_kind):
    """The corpus of one shape, built once per session and shared (Items are immutable: bytes and ints)."""
    key = (log_n, log_b, q, g, K, hash_kind)
    if key not in _corpora:
        _corpora[key] = variants(ref_proofs(orc, log_n, log_b, q, g, K, hash_kind), fields(log_n, log_b, q, g, K))
    return _corpora[key]


def cpu_checks(lib, items, log_n, log_b, q, g, K, hash_kind, strict):
    """zk_verify_fold's check number for every item, as an int32 array."""
    import ctypes as C
    out = np.zeros(len(items), dtype=np.int32)
    for i, it in enumerate(items):
        c = C.c_int32(12345)
        rc = lib.zk_verify_fold(it.data, len(it.data), it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K, C.byref(c))
        assert rc == (0 if c.value == 0 else -6), (it.label, rc, c.value)
        out[i] = c.value
    return out
