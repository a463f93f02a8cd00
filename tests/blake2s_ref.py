"""Trees, paths and whole proofs with BLAKE2s-256 as the Merkle hash (ZK_HASH_BLAKE2S = 2), built without the library
(tests/test_blake2s.py, tests/test_gpu_blake2s.py).

Every digest here is hashlib.blake2s: a leaf is the hash of its slots, 4 bytes big-endian each (one slot: the one-value leaf), a node
the hash of left || right.  What does not depend on the Merkle hash is imported: the channel (SHA-256 on hashlib whatever the tree
hash), the groups, the folds through the oracle's primitives, the final polynomial, the lengths, the Fiat-Shamir replay and the walk
along a heap.  Only what hard-codes the hash in fold_ref / coset_ref / stop_ref is restated: the trees, the commitments and the
verifier's path checks.  One model covers every setting: K = 1..3, one-value or coset leaves, D = 0 or an early stop."""
import functools
import hashlib
import struct

import numpy as np

import grind_ref
import stop_ref
from coset_ref import path
from fold_ref import GEN_W, P, RefProof, _Channel, _inv, _Reader, _Short, fold_layer, groups
from stop_ref import final_coefficients, proof_len, replay

HASH_KIND = 2


def digest(msg):
    return hashlib.blake2s(bytes(msg)).digest()


def leaf_hash(slots):
    """The digest of a leaf of len(slots) in (1, 2, 4, 8) values."""
    return digest(b"".join(struct.pack(">I", int(v)) for v in slots))


def node_hash(left, right):
    return digest(bytes(left) + bytes(right))


def tree(layer, steps=0):
    """Heap (merkle.rs:14-51) over `layer` with 2^steps-wide coset leaves (0: one value per leaf), as a [2 m - 1, 32] uint8 array."""
    s, m = 1 << steps, len(layer) >> steps
    heap = [None] * (2 * m - 1)
    for c in range(m):
        heap[m - 1 + c] = leaf_hash([layer[c + u * m] for u in range(s)])
    for i in range(m - 2, -1, -1):
        heap[i] = node_hash(heap[2 * i + 1], heap[2 * i + 2])
    return np.frombuffer(b"".join(heap), dtype=np.uint8).reshape(2 * m - 1, 32)


def root_from_leaf(slots, leaf, pth):
    """merkle.rs:82-110 from the slots of leaf `leaf` and its path (sibling of the leaf first)."""
    cur, i = leaf_hash(slots), leaf + (1 << len(pth)) - 1
    for sib in pth:
        cur = node_hash(cur, sib) if i & 1 else node_hash(sib, cur)
        i = (i - 1) >> 1
    return cur


class Committed:
    """layers[id], trees[id], roots[id] for the committed ids, betas[r0], alphas, coef (the free term alone when D = 0), and the
    channel after the free term / the coefficients."""


@functools.lru_cache(maxsize=16)
def committed(orc, log_n, log_b, K, coset, D, a1=3141592, prefix=b""):
    assert stop_ref.admissible(log_n, log_b, D)
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    Rp = log_n - D
    grp = groups(Rp, K)
    c = Committed()
    c.public_last, c.layers, c.trees, c.roots, c.betas = r.public_last, {}, {}, {}, {}
    ch = _Channel(prefix)

    def commit_layer(i, vals, steps):
        c.layers[i] = np.array(vals, dtype=np.uint32)
        c.trees[i] = tree(c.layers[i], steps)
        c.roots[i] = bytes(c.trees[i][0])
        ch.commit(c.roots[i])

    commit_layer(0, r.f_eval, 0)
    c.alphas = [ch.get_u32() for _ in range(3)]
    commit_layer(1, orc.compose(r.f_eval, log_n, log_b, c.alphas, r.public_last), grp[0][1] if coset else 0)
    for j, (r0, steps) in enumerate(grp):
        beta = c.betas[r0] = ch.get_u32()
        out = fold_layer(orc, c.layers[1 + r0], log_n, log_b, r0, steps, beta)
        if D and j + 1 == len(grp):
            c.layers[1 + Rp] = np.array(out, dtype=np.uint32)   # the stopped layer: no tree, no root
        else:
            commit_layer(1 + r0 + steps, out, grp[j + 1][1] if coset and j + 1 < len(grp) else 0)
    if D:
        c.coef = final_coefficients(c.layers[1 + Rp], log_n, log_b, D)
    else:
        last = c.layers[1 + log_n]
        assert len(last) == 1 << log_b and len(set(int(v) for v in last)) == 1
        c.coef = [int(last[0])]
    ch.commit(b"".join(struct.pack("<I", v) for v in c.coef))      # one commit: the free term, or the 4 * 2^D bytes of coefficients
    c.prefix_state, c.prefix_data = ch.state, bytes(ch.data)
    return c


def proof(orc, log_n, log_b, q=1, K=1, coset=False, D=0, bits=0, a1=3141592, prefix=b""):
    """The proof of fibsq(1, a1) with BLAKE2s trees: .data (the prefix included), .state, .public_last, .nonce, .raws, .c, .coef,
    .queries_at (offset of the first query's first tuple in .data)."""
    c = committed(orc, log_n, log_b, K, bool(coset), D, a1, prefix)
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = c.prefix_state, bytearray(c.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce, out.coef = c, c.public_last, None, list(c.coef)
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]
    out.queries_at = len(ch.data)
    for raw in raws:
        x = raw % (N - 2 * B)
        for lid, idx in ((0, x), (0, x + B), (0, x + 2 * B)) + (() if coset else ((1, x),)):
            ch.commit(struct.pack("<IQ", int(c.layers[lid][idx]), L) + b"".join(path(c.trees[lid], idx)))
        for r0, steps in groups(log_n - D, K):
            layer, tr = c.layers[1 + r0], c.trees[1 + r0]
            if coset:
                m = (N >> r0) >> steps
                leaf = x % m
                ch.commit(b"".join(struct.pack("<I", int(layer[leaf + u * m])) for u in range(1 << steps))
                          + struct.pack("<Q", L - r0 - steps) + b"".join(path(tr, leaf)))
            else:
                s, size = 1 << steps, N >> r0
                idx = [(x % size + t * (size // s)) % size for t in range(s)]
                ch.commit(b"".join(struct.pack("<I", int(layer[i])) for i in idx)
                          + b"".join(struct.pack("<Q", L - r0) + b"".join(path(tr, i)) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    return out


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D):
    """The check number of the verifier under `hash_kind`: the models of stop_ref for SHA-256 and the field hash, the one below for
    BLAKE2s.  Strict (the replay first) when state is not None."""
    if hash_kind != HASH_KIND:
        return stop_ref.verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D)
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K, coset, D)
        if rc:
            return rc
    if D and (not stop_ref.admissible(log_n, log_b, D) or len(data) != proof_len(log_n, log_b, q, bits, K, coset, D)):
        return -1                                           # a stopped proof of another length is -1, strict or not
    return _verify(data, log_n, log_b, public_last, q, bits, K, coset, D)


def _verify(data, log_n, log_b, public_last, q, bits, K, coset, D):
    """stop_ref._verify (D = 0: fold_ref._verify / coset_ref._verify) with the path checks on hashlib.blake2s."""
    n, L, Rp = 1 << log_n, log_n + log_b, log_n - D
    N, B = 1 << L, 1 << log_b
    grp = groups(Rp, K)
    G, nf = len(grp), 3 if coset else 4
    rd = _Reader(data)
    try:
        f_root = rd.take(32)
        alpha = [rd.u32() for _ in range(3)]
        roots = [rd.take(32)]
        betas = []
        for j in range(G):
            betas.append(rd.u32())
            if not D or j + 1 < G:
                roots.append(rd.take(32))
        coef = [rd.u32() for _ in range(1 << D)]            # D = 0: the free term, compared unreduced
        if bits:
            rd.take(8)
        raws = [rd.u32() for _ in range(q)]
    except _Short:
        return -1
    g, h = pow(GEN_W, (P - 1) >> log_n, P), pow(GEN_W, (P - 1) >> L, P)
    inv2 = _inv(2)
    for raw in raws:
        try:
            fv, fp = [], []
            for _ in range(nf):
                fv.append(rd.u32())
                fp.append(rd.path())
            lv, lp = [], []
            for r0, steps in grp:
                lv.append([rd.u32() for _ in range(1 << steps)])
                lp.append([rd.path() for _ in range(1 if coset else 1 << steps)])
        except _Short:
            return -1
        tp = raw % (N - 2 * B)

        def val(j, t):                                      # value t of group j: as sent, or slot (rot + t) % s of its leaf
            if not coset:
                return lv[j][t]
            r0, steps = grp[j]
            size, s = N >> r0, 1 << steps
            return lv[j][((tp % size) // (size // s) + t) % s]

        x = GEN_W * pow(h, tp, P) % P
        f_x, f_gx, f_ggx = fv[0] % P, fv[1] % P, fv[2] % P
        gm1 = _inv(g)
        gm2, gm3 = gm1 * gm1 % P, gm1 * gm1 * gm1 % P
        p0 = (f_x - 1) * _inv((x - 1) % P) % P
        p1 = (f_x - public_last % P) * _inv((x - gm2) % P) % P
        num = (f_ggx - f_gx * f_gx - f_x * f_x) % P
        den = (pow(x, n, P) - 1) * _inv((x - gm3) * (x - gm2) * (x - gm1) % P) % P
        p2 = num * _inv(den) % P
        if (alpha[0] % P * p0 + alpha[1] % P * p1 + alpha[2] % P * p2) % P != (val(0, 0) if coset else fv[3]):
            return -2
        if any(len(p) != L for p in fp):
            return -3
        for i, (idx, root) in enumerate(((tp, f_root), (tp + B, f_root), (tp + 2 * B, f_root), (tp, roots[0]))[:nf]):
            if root_from_leaf([fv[i]], idx, fp[i]) != root:
                return -(4 + i)
        for j, (r0, steps) in enumerate(grp):
            v = [val(j, t) % P for t in range(1 << steps)]
            xk, om, bk = pow(x, 1 << r0, P), pow(h, N >> steps, P), betas[j] % P
            for _ in range(steps):
                cnt = len(v) // 2
                v = [((v[t] + v[t + cnt]) * inv2 + bk * (v[t] - v[t + cnt]) * _inv(2 * xk * pow(om, t, P) % P)) % P for t in range(cnt)]
                xk, om, bk = xk * xk % P, om * om % P, bk * bk % P
            if j + 1 < G:
                expect = val(j + 1, 0)
            elif not D:
                expect = coef[0]
            else:                                           # p at the query's point of the stopped layer, by Horner
                xs, expect = pow(x, 1 << Rp, P), 0
                for ck in reversed(coef):
                    expect = (expect * xs + ck % P) % P
            if v[0] != expect:
                return -(100 + j)
        for j, (r0, steps) in enumerate(grp):
            s, size = 1 << steps, N >> r0
            if coset:
                m = size >> steps
                if len(lp[j][0]) != L - r0 - steps:
                    return -(200 + j)
                if root_from_leaf(lv[j], tp % m, lp[j][0]) != roots[j]:
                    return -(300 + j)
                continue
            if any(len(p) != L - r0 for p in lp[j]):
                return -(200 + j)
            for t in range(s):
                if root_from_leaf([lv[j][t]], (tp % size + t * (size // s)) % size, lp[j][t]) != roots[j]:
                    return -(300 + j) if t == 0 else -(400 + j)
    return -8 if rd.p != len(data) else 0
