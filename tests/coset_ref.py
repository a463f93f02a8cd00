"""Proofs with coset leaves built without the library, and a plain-Python verifier of that format
(tests/test_coset_leaves.py, tests/test_gpu_coset_leaves.py; DESIGN.md 7d "Coset leaves").

Layers come from the oracle's primitives exactly as in fold_ref.committed.  The tree over the input layer of a group (id 1 + r0,
len values, s = 2^steps) has len / s leaves, leaf c holding the slots layer[c + u len / s]; it is built here in plain Python: a
leaf is hashlib.sha256 over the slots as 4 bytes big-endian each, or, for the field hash, orc.fieldhash_permute of
(slot_0 .. slot_{s-1}, 0, ..., 0, s) plus the feed-forward, truncated to 8 elements; inner nodes are orc.node_hash.  Tree 0 (f)
and the tree over the last layer keep one-value leaves (orc.merkle_build).  The channel runs on hashlib."""
import functools
import hashlib
import struct

import numpy as np

import grind_ref
from fold_ref import GEN_W, P, RefProof, _Channel, _inv, _Reader, _Short, fold_layer, groups


def proof_len(log_n, log_b, q, bits, K):
    L = log_n + log_b
    grp = groups(log_n, K)
    per_query = 4 + 3 * (12 + 32 * L) + sum(4 * (1 << s) + 8 + 32 * (L - r0 - s) for r0, s in grp)
    return 32 + 12 + 32 + 36 * len(grp) + 4 + (8 if bits else 0) + q * per_query


def leaf_hash(orc, slots, hash_kind):
    """The digest of a leaf of len(slots) in (1, 2, 4, 8) values."""
    s = len(slots)
    if hash_kind == 0:
        return hashlib.sha256(b"".join(struct.pack(">I", int(v)) for v in slots)).digest()
    state = [int(v) % P for v in slots] + [0] * (15 - s) + [s]
    out = orc.fieldhash_permute(np.array(state, dtype=np.uint32))
    return b"".join(struct.pack(">I", (int(out[i]) + state[i]) % P) for i in range(8))


def tree(orc, layer, steps, hash_kind):
    """Heap of the tree with 2^steps-wide coset leaves over `layer`, as a [2 m - 1, 32] uint8 array (m = len / 2^steps).
    The caller has selected the hash with orc.set_hash(hash_kind) (orc.node_hash follows it)."""
    s, m = 1 << steps, len(layer) >> steps
    heap = [None] * (2 * m - 1)
    for c in range(m):
        heap[m - 1 + c] = leaf_hash(orc, [layer[c + u * m] for u in range(s)], hash_kind)
    for i in range(m - 2, -1, -1):
        heap[i] = orc.node_hash(heap[2 * i + 1], heap[2 * i + 2])
    return np.frombuffer(b"".join(heap), dtype=np.uint8).reshape(2 * m - 1, 32)


def path(nodes, leaf):
    """merkle.rs:54-71 on a heap: the sibling of the leaf first, the child of the root last."""
    i, out = leaf + len(nodes) // 2, []
    while i:
        out.append(bytes(nodes[i + 1 if i & 1 else i - 1]))
        i = (i - 1) >> 1
    return out


def root_from_leaf(orc, slots, leaf, pth, hash_kind):
    """merkle.rs:82-110 from the slots of coset leaf `leaf`; orc.set_hash(hash_kind) is in force."""
    cur, i = leaf_hash(orc, slots, hash_kind), leaf + (1 << len(pth)) - 1
    for sib in pth:
        cur = orc.node_hash(cur, sib) if i & 1 else orc.node_hash(sib, cur)
        i = (i - 1) >> 1
    return cur


class Committed:
    """layers[id], trees[id] (heaps), steps[id] (leaf width of tree id), roots[id], betas[r0], alphas, and the channel after the free term."""


@functools.lru_cache(maxsize=8)
def committed(orc, log_n, log_b, hash_kind, K, a1=3141592, prefix=b""):
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    grp = groups(log_n, K)
    c = Committed()
    c.public_last, c.layers, c.trees, c.steps, c.roots, c.betas = r.public_last, {}, {}, {}, {}, {}
    ch = _Channel(prefix)
    orc.set_hash(hash_kind)
    try:
        def commit_layer(i, vals, steps):
            c.layers[i] = np.array(vals, dtype=np.uint32)
            c.steps[i] = steps
            c.trees[i] = tree(orc, c.layers[i], steps, hash_kind) if steps else orc.merkle_build(c.layers[i])
            c.roots[i] = bytes(c.trees[i][0])
            ch.commit(c.roots[i])

        commit_layer(0, r.f_eval, 0)
        c.alphas = [ch.get_u32() for _ in range(3)]
        commit_layer(1, orc.compose(r.f_eval, log_n, log_b, c.alphas, r.public_last), grp[0][1])
        for j, (r0, steps) in enumerate(grp):
            beta = c.betas[r0] = ch.get_u32()
            commit_layer(1 + r0 + steps, fold_layer(orc, c.layers[1 + r0], log_n, log_b, r0, steps, beta), grp[j + 1][1] if j + 1 < len(grp) else 0)
    finally:
        orc.set_hash(0)
    last = c.layers[1 + log_n]
    assert len(last) == 1 << log_b and len(set(int(v) for v in last)) == 1
    c.free_term = int(last[0])
    ch.commit(struct.pack("<I", c.free_term))
    c.prefix_state, c.prefix_data = ch.state, bytes(ch.data)
    return c


def coset_proof(orc, log_n, log_b, q, hash_kind, K, bits=0, a1=3141592, prefix=b""):
    """The coset-leaf proof of fibsq(1, a1) folded by 2^K: .data (the prefix included), .state, .public_last, .nonce, .raws, .c."""
    c = committed(orc, log_n, log_b, hash_kind, K, a1, prefix)
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = c.prefix_state, bytearray(c.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce = c, c.public_last, None
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]
    for raw in raws:
        x = raw % (N - 2 * B)
        for idx in (x, x + B, x + 2 * B):
            ch.commit(struct.pack("<IQ", int(c.layers[0][idx]), L) + b"".join(path(c.trees[0], idx)))
        for r0, steps in groups(log_n, K):
            m = (N >> r0) >> steps
            leaf = x % m
            ch.commit(b"".join(struct.pack("<I", int(c.layers[1 + r0][leaf + u * m])) for u in range(1 << steps))
                      + struct.pack("<Q", L - r0 - steps) + b"".join(path(c.trees[1 + r0], leaf)))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    return out


def regions(log_n, log_b, q, bits, K):
    """[(name, offset, length)] of every field of a coset proof, in wire order (what the tampering tests flip a byte in)."""
    L, out, o = log_n + log_b, [], 0

    def add(name, n):
        nonlocal o
        out.append((name, o, n))
        o += n

    add("f_root", 32)
    for i in range(3):
        add(f"alpha{i}", 4)
    add("root0", 32)
    for j, _ in enumerate(groups(log_n, K)):
        add(f"beta{j}", 4)
        add(f"root{j + 1}", 32)
    add("free_term", 4)
    if bits:
        add("nonce", 8)
    for k in range(q):
        add(f"raw{k}", 4)
    for k in range(q):
        for i in range(3):
            add(f"q{k}.f{i}.value", 4)
            add(f"q{k}.f{i}.count", 8)
            add(f"q{k}.f{i}.path", 32 * L)
        for j, (r0, steps) in enumerate(groups(log_n, K)):
            for u in range(1 << steps):
                add(f"q{k}.g{j}.slot{u}", 4)
            add(f"q{k}.g{j}.count", 8)
            add(f"q{k}.g{j}.path", 32 * (L - r0 - steps))
    assert o == proof_len(log_n, log_b, q, bits, K)
    return out


# ---- the verifier, in plain Python ---------------------------------------------------------------------------------------------
def replay(data, state, log_n, log_b, q, bits, K):
    """The Fiat-Shamir replay: 0, -1 (length), -(1000 + k) for the k-th challenge, -1998 for the nonce, -1999 for the state."""
    L = log_n + log_b
    if len(data) != proof_len(log_n, log_b, q, bits, K):
        return -1
    ch, rd, k = _Channel(), _Reader(data), 0

    def challenge():
        want = struct.unpack(">I", ch.state[:4])[0]
        b = rd.take(4)
        if struct.unpack("<I", b)[0] != want:
            return False
        ch.commit(b)
        return True

    ch.commit(rd.take(32))
    for _ in range(3):
        k += 1
        if not challenge():
            return -(1000 + k)
    ch.commit(rd.take(32))
    for _ in groups(log_n, K):
        k += 1
        if not challenge():
            return -(1000 + k)
        ch.commit(rd.take(32))
    ch.commit(rd.take(4))
    if bits:
        ch.commit(rd.take(8))
        if struct.unpack(">I", ch.state[:4])[0] >> (32 - bits):
            return -1998
    for _ in range(q):
        k += 1
        if not challenge():
            return -(1000 + k)
    for _ in range(q):
        for _ in range(3):
            ch.commit(rd.take(12 + 32 * L))
        for r0, steps in groups(log_n, K):
            ch.commit(rd.take(4 * (1 << steps) + 8 + 32 * (L - r0 - steps)))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K):
    """The check number of the coset-leaf verifier: strict (the replay first) when state is not None."""
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K)
        if rc:
            return rc
    orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K)
    finally:
        orc.set_hash(0)


def _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K):
    n, L = 1 << log_n, log_n + log_b
    N, B = 1 << L, 1 << log_b
    grp = groups(log_n, K)
    G = len(grp)
    rd = _Reader(data)
    try:
        f_root = rd.take(32)
        alpha = [rd.u32() for _ in range(3)]
        roots = [rd.take(32)]
        betas = []
        for _ in grp:
            betas.append(rd.u32())
            roots.append(rd.take(32))
        free_term = rd.u32()
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
            for _ in range(3):
                fv.append(rd.u32())
                fp.append(rd.path())
            lv, lp = [], []
            for r0, steps in grp:
                lv.append([rd.u32() for _ in range(1 << steps)])
                lp.append(rd.path())
        except _Short:
            return -1
        tp = raw % (N - 2 * B)

        def val(j, t):                                      # value t of group j: slot (rot + t) % s of its leaf
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
        if (alpha[0] % P * p0 + alpha[1] % P * p1 + alpha[2] % P * p2) % P != val(0, 0):
            return -2
        if any(len(p) != L for p in fp):
            return -3
        for i, idx in enumerate((tp, tp + B, tp + 2 * B)):
            if root_from_leaf(orc, [fv[i]], idx, fp[i], hash_kind) != f_root:
                return -(4 + i)
        for j, (r0, steps) in enumerate(grp):
            v = [val(j, t) % P for t in range(1 << steps)]
            xk, om, bk = pow(x, 1 << r0, P), pow(h, N >> steps, P), betas[j] % P
            for _ in range(steps):
                cnt = len(v) // 2
                v = [((v[t] + v[t + cnt]) * inv2 + bk * (v[t] - v[t + cnt]) * _inv(2 * xk * pow(om, t, P) % P)) % P for t in range(cnt)]
                xk, om, bk = xk * xk % P, om * om % P, bk * bk % P
            if v[0] != (val(j + 1, 0) if j + 1 < G else free_term):
                return -(100 + j)
        for j, (r0, steps) in enumerate(grp):
            m = (N >> r0) >> steps
            if len(lp[j]) != L - r0 - steps:
                return -(200 + j)
            if root_from_leaf(orc, lv[j], tp % m, lp[j], hash_kind) != roots[j]:
                return -(300 + j)
    return -8 if rd.p != len(data) else 0
