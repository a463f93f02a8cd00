"""Proofs that stop FRI early (zk_ctx_set_fri_stop; DESIGN.md 7d "Early stop") built without the library, and a plain-Python
verifier of that format (tests/test_fri_stop.py, tests/test_gpu_fri_stop.py).

D = stop_log > 0: only the first R' = log_n - D rounds are folded, in the groups of R' (fold_ref.groups(R', K)).  Layers come from the
oracle's primitives as in fold_ref / coset_ref, trees from orc.merkle_build (one-value leaves) or coset_ref.tree (coset leaves).  The
output of the last group, layer id 1 + R', holds M = 2^(D + log_b) evaluations of a polynomial p of degree < 2^D at
X_i = (w h^i)^(2^R'); it gets no tree.  Its 2^D monomial coefficients -- an O(M 2^D) inverse DFT written out in Python integers,
checked by evaluating p at all M points -- are committed in one piece in place of the last root and the free term.  D = 0 is
fold_ref / coset_ref."""
import functools
import struct

import numpy as np

import coset_ref
import fold_ref
import grind_ref
from fold_ref import GEN_W, P, RefProof, _Channel, _inv, _Reader, _Short, fold_layer, groups

MAX_STOP, MAX_LAYER_LOG = 8, 12


def admissible(log_n, log_b, D):
    return D == 0 or (1 <= D <= MAX_STOP and D <= log_n - 1 and D + log_b <= MAX_LAYER_LOG)


def proof_len(log_n, log_b, q, bits, K, coset, D):
    if D == 0:
        return (coset_ref if coset else fold_ref).proof_len(log_n, log_b, q, bits, K)
    L, grp = log_n + log_b, groups(log_n - D, K)
    if coset:
        per_query = 4 + 3 * (12 + 32 * L) + sum(4 * (1 << s) + 8 + 32 * (L - r0 - s) for r0, s in grp)
    else:
        per_query = 4 + 4 * (12 + 32 * L) + sum((1 << s) * (12 + 32 * (L - r0)) for r0, s in grp)
    return 32 + 12 + 32 + 36 * (len(grp) - 1) + 4 + 4 * (1 << D) + (8 if bits else 0) + q * per_query


def final_coefficients(layer, log_n, log_b, D):
    """The 2^D coefficients of the polynomial of degree < 2^D whose values at X_i = (w h^i)^(2^R'), i < M, are `layer`."""
    L, Rp = log_n + log_b, log_n - D
    M = 1 << (D + log_b)
    assert len(layer) == M
    h = pow(GEN_W, (P - 1) >> L, P)
    s, om = pow(GEN_W, 1 << Rp, P), pow(h, 1 << Rp, P)          # X_i = s om^i, om of order M
    assert pow(om, M, P) == 1 and pow(om, M // 2, P) == P - 1
    vals = [int(v) for v in layer]
    minv, sinv, ominv = _inv(M), _inv(s), _inv(om)
    coef = []
    for k in range(1 << D):
        step, x, acc = pow(ominv, k, P), 1, 0
        for v in vals:
            acc += v * x
            x = x * step % P
        coef.append(acc % P * minv % P * pow(sinv, k, P) % P)
    assert np.array_equal(evaluate(coef, points(log_n, log_b, Rp)), np.array(vals, dtype=np.uint64))   # p reproduces the whole layer
    return coef


def points(log_n, log_b, r):
    """X_i = (w h^i)^(2^r), i < N >> r, as a uint64 array: the evaluation points of FRI layer id 1 + r."""
    L = log_n + log_b
    s, om = pow(GEN_W, 1 << r, P), pow(pow(GEN_W, (P - 1) >> L, P), 1 << r, P)
    out, x = np.zeros(1 << (L - r), dtype=np.uint64), s
    for i in range(len(out)):
        out[i] = x
        x = x * om % P
    return out


def evaluate(coef, xs):
    """Horner over a vector of points in numpy uint64 (every product of two residues fits 64 bits)."""
    acc = np.zeros(len(xs), dtype=np.uint64)
    for c in reversed([int(v) for v in coef]):
        acc = (acc * xs + np.uint64(c)) % np.uint64(P)
    return acc


class Committed:
    """layers[id], trees[id], roots[id] for the committed ids, betas[r0], alphas, coef, and the channel after the coefficients."""


@functools.lru_cache(maxsize=8)
def committed(orc, log_n, log_b, hash_kind, K, coset, D, a1=3141592, prefix=b""):
    assert D > 0 and admissible(log_n, log_b, D)
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    Rp = log_n - D
    grp = groups(Rp, K)
    c = Committed()
    c.public_last, c.layers, c.trees, c.roots, c.betas = r.public_last, {}, {}, {}, {}
    ch = _Channel(prefix)
    orc.set_hash(hash_kind)
    try:
        def commit_layer(i, vals, steps):
            c.layers[i] = np.array(vals, dtype=np.uint32)
            c.trees[i] = coset_ref.tree(orc, c.layers[i], steps, hash_kind) if steps else orc.merkle_build(c.layers[i])
            c.roots[i] = bytes(c.trees[i][0])
            ch.commit(c.roots[i])

        commit_layer(0, r.f_eval, 0)
        c.alphas = [ch.get_u32() for _ in range(3)]
        commit_layer(1, orc.compose(r.f_eval, log_n, log_b, c.alphas, r.public_last), grp[0][1] if coset else 0)
        for j, (r0, steps) in enumerate(grp):
            beta = c.betas[r0] = ch.get_u32()
            out = fold_layer(orc, c.layers[1 + r0], log_n, log_b, r0, steps, beta)
            if j + 1 < len(grp):
                commit_layer(1 + r0 + steps, out, grp[j + 1][1] if coset else 0)
            else:
                c.layers[1 + Rp] = np.array(out, dtype=np.uint32)   # the stopped layer: no tree, no root
    finally:
        orc.set_hash(0)
    c.coef = final_coefficients(c.layers[1 + Rp], log_n, log_b, D)
    ch.commit(b"".join(struct.pack("<I", v) for v in c.coef))      # one commit of 4 * 2^D bytes
    c.prefix_state, c.prefix_data = ch.state, bytes(ch.data)
    return c


def stop_proof(orc, log_n, log_b, q, hash_kind, K, coset, D, bits=0, a1=3141592, prefix=b""):
    """The proof of fibsq(1, a1) folded by 2^K, with or without coset leaves, stopped at degree < 2^D: .data (the prefix included),
    .state, .public_last, .nonce, .raws, .c (Committed), .coef."""
    if D == 0:
        ref = (coset_ref.coset_proof if coset else fold_ref.fold_proof)(orc, log_n, log_b, q, hash_kind, K, bits, a1, prefix)
        ref.coef = [ref.c.free_term]
        return ref
    c = committed(orc, log_n, log_b, hash_kind, K, bool(coset), D, a1, prefix)
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = c.prefix_state, bytearray(c.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce, out.coef = c, c.public_last, None, list(c.coef)
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]
    for raw in raws:
        x = raw % (N - 2 * B)
        for lid, idx in ((0, x), (0, x + B), (0, x + 2 * B)) + (() if coset else ((1, x),)):
            ch.commit(struct.pack("<IQ", int(c.layers[lid][idx]), L) + b"".join(coset_ref.path(c.trees[lid], idx)))
        for r0, steps in groups(log_n - D, K):
            layer, tree = c.layers[1 + r0], c.trees[1 + r0]
            if coset:
                m = (N >> r0) >> steps
                leaf = x % m
                ch.commit(b"".join(struct.pack("<I", int(layer[leaf + u * m])) for u in range(1 << steps))
                          + struct.pack("<Q", L - r0 - steps) + b"".join(coset_ref.path(tree, leaf)))
            else:
                s, size = 1 << steps, N >> r0
                idx = [(x % size + t * (size // s)) % size for t in range(s)]
                ch.commit(b"".join(struct.pack("<I", int(layer[i])) for i in idx)
                          + b"".join(struct.pack("<Q", L - r0) + b"".join(coset_ref.path(tree, i)) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    return out


def regions(log_n, log_b, q, bits, K, coset, D):
    """[(name, offset, length)] of every field of a stopped proof (D > 0) in wire order: what the tampering tests flip a byte in."""
    assert D > 0
    L, grp, out, o = log_n + log_b, groups(log_n - D, K), [], 0

    def add(name, n):
        nonlocal o
        out.append((name, o, n))
        o += n

    add("f_root", 32)
    for i in range(3):
        add(f"alpha{i}", 4)
    add("root0", 32)
    for j in range(len(grp)):
        add(f"beta{j}", 4)
        if j + 1 < len(grp):
            add(f"root{j + 1}", 32)
    for k in range(1 << D):
        add(f"coef{k}", 4)
    if bits:
        add("nonce", 8)
    for k in range(q):
        add(f"raw{k}", 4)
    for k in range(q):
        for i in range(3 if coset else 4):
            add(f"q{k}.f{i}.value", 4)
            add(f"q{k}.f{i}.count", 8)
            add(f"q{k}.f{i}.path", 32 * L)
        for j, (r0, steps) in enumerate(grp):
            if coset:
                for u in range(1 << steps):
                    add(f"q{k}.g{j}.slot{u}", 4)
                add(f"q{k}.g{j}.count", 8)
                add(f"q{k}.g{j}.path", 32 * (L - r0 - steps))
            else:
                for t in range(1 << steps):
                    add(f"q{k}.g{j}.value{t}", 4)
                for t in range(1 << steps):
                    add(f"q{k}.g{j}.count{t}", 8)
                    add(f"q{k}.g{j}.path{t}", 32 * (L - r0))
    assert o == proof_len(log_n, log_b, q, bits, K, coset, D)
    return out


# ---- the verifier, in plain Python ---------------------------------------------------------------------------------------------
def replay(data, state, log_n, log_b, q, bits, K, coset, D):
    """The Fiat-Shamir replay: 0, -1 (length or limits), -(1000 + k) for the k-th of the 3 + G' + q challenges, -1998 for the nonce
    (checked on the state after the coefficients and the nonce), -1999 for the state."""
    if D == 0:
        return (coset_ref if coset else fold_ref).replay(data, state, log_n, log_b, q, bits, K)
    if not admissible(log_n, log_b, D) or len(data) != proof_len(log_n, log_b, q, bits, K, coset, D):
        return -1
    L, grp = log_n + log_b, groups(log_n - D, K)
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
    for j in range(len(grp)):
        k += 1
        if not challenge():
            return -(1000 + k)
        if j + 1 < len(grp):
            ch.commit(rd.take(32))
    ch.commit(rd.take(4 << D))                              # the coefficients, in one piece
    if bits:
        ch.commit(rd.take(8))
        if struct.unpack(">I", ch.state[:4])[0] >> (32 - bits):
            return -1998
    for _ in range(q):
        k += 1
        if not challenge():
            return -(1000 + k)
    for _ in range(q):
        for _ in range(3 if coset else 4):
            ch.commit(rd.take(12 + 32 * L))
        for r0, steps in grp:
            ch.commit(rd.take(4 * (1 << steps) + 8 + 32 * (L - r0 - steps) if coset else (1 << steps) * (12 + 32 * (L - r0))))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D):
    """The check number of the verifier of stopped proofs: strict (the replay first) when state is not None."""
    if D == 0:
        return (coset_ref if coset else fold_ref).verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K)
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K, coset, D)
        if rc:
            return rc
    if not admissible(log_n, log_b, D) or len(data) != proof_len(log_n, log_b, q, bits, K, coset, D):
        return -1                                           # a stopped proof of another length is -1, strict or not
    orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D)
    finally:
        orc.set_hash(0)


def _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D):
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
            if j + 1 < G:
                roots.append(rd.take(32))
        coef = [rd.u32() % P for _ in range(1 << D)]        # reduced on reading, as raw challenges are
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
            if coset_ref.root_from_leaf(orc, [fv[i]], idx, fp[i], hash_kind) != root:
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
            else:                                           # p at the query's point of the stopped layer, by Horner
                xs, expect = pow(x, 1 << Rp, P), 0
                for ck in reversed(coef):
                    expect = (expect * xs + ck) % P
            if v[0] != expect:
                return -(100 + j)
        for j, (r0, steps) in enumerate(grp):
            s, size = 1 << steps, N >> r0
            if coset:
                m = size >> steps
                if len(lp[j][0]) != L - r0 - steps:
                    return -(200 + j)
                if coset_ref.root_from_leaf(orc, lv[j], tp % m, lp[j][0], hash_kind) != roots[j]:
                    return -(300 + j)
                continue
            if any(len(p) != L - r0 for p in lp[j]):
                return -(200 + j)
            for t in range(s):
                if coset_ref.root_from_leaf(orc, [lv[j][t]], (tp % size + t * (size // s)) % size, lp[j][t], hash_kind) != roots[j]:
                    return -(300 + j) if t == 0 else -(400 + j)
    return -8 if rd.p != len(data) else 0
