"""Proofs with Merkle caps (zk_ctx_set_merkle_cap) built without the library, and a plain-Python verifier of that
format (tests/test_merkle_cap.py, tests/test_gpu_merkle_cap.py).

cap_log = c: a tree over 2^lg leaves is committed by the 2^ce digests of depth ce = min(c, lg - 1), heap nodes 2^ce - 1 .. 2^(ce+1) - 2 in
one channel commit, and a path into it carries the lg - ce siblings below that depth.  The layers, the folds, the final polynomial, the
channel, the groups and the heaps are those of fold_ref / coset_ref / stop_ref / blake2s_ref: this module hashes nothing of its own, it
reads the cap of a tree out of the heap those build and cuts the paths they walk.  What it cannot take over is a finished run: the
challenges are drawn from the commitments, so with c > 0 every layer after f differs from the cap-0 run and the transcript is walked
again here, with the same primitives.  One model covers every setting: hash 0, 1 (the oracle's trees) and 2 (blake2s_ref's), K = 1..3,
one-value or coset leaves, D = 0 or an early stop.  With c = 0 the bytes are stop_ref.stop_proof's / blake2s_ref.proof's."""
import functools
import struct

import numpy as np

import blake2s_ref
import coset_ref
import grind_ref
import stop_ref
from fold_ref import GEN_W, P, RefProof, _Channel, _inv, _Reader, _Short, fold_layer, groups

MAX_CAP = 8


def c_eff(c, lg):
    """The depth a tree of 2^lg leaves is committed at."""
    return min(c, lg - 1)


def trees(log_n, log_b, K, coset, D):
    """[(tree id, lg)] of the committed trees in commit order: f, then the tree over the input layer of every group (coset leaves count
    once), then, when D = 0, the never-opened tree over the last layer."""
    L, grp = log_n + log_b, groups(log_n - D, K)
    out = [(0, L)] + [(1 + r0, L - r0 - (steps if coset else 0)) for r0, steps in grp]
    if D == 0:
        out.append((1 + log_n, log_b))
    return out


def paths_into(log_n, log_b, K, coset, D):
    """{tree id: paths per query}."""
    n = {0: 3}
    for j, (r0, steps) in enumerate(groups(log_n - D, K)):
        n[1 + r0] = (1 if coset else 1 << steps) + (1 if j == 0 and not coset else 0)
    return n


def proof_len(log_n, log_b, q, bits, K, coset, D, c):
    """The issue's formula: the cap-0 length, plus 32 (2^ce - 1) in the head per committed tree, minus 32 ce per path into it."""
    n = stop_ref.proof_len(log_n, log_b, q, bits, K, coset, D)
    per_tree = paths_into(log_n, log_b, K, coset, D)
    for tid, lg in trees(log_n, log_b, K, coset, D):
        ce = c_eff(c, lg)
        n += 32 * ((1 << ce) - 1) - q * per_tree.get(tid, 0) * 32 * ce
    return n


def cap_of(heap, ce):
    """The 2^ce digests of depth ce of a heap, as bytes."""
    return b"".join(bytes(heap[i]) for i in range((1 << ce) - 1, (2 << ce) - 1))


def cut_path(heap, leaf, ce):
    """coset_ref.path without its last ce digests: the siblings from the leaf up to depth ce + 1."""
    p = coset_ref.path(heap, leaf)
    return p[:len(p) - ce]


def _tree(orc, layer, steps, hash_kind):
    if hash_kind == blake2s_ref.HASH_KIND:
        return blake2s_ref.tree(layer, steps)
    return coset_ref.tree(orc, layer, steps, hash_kind) if steps else orc.merkle_build(layer)


def _climb(orc, slots, leaf, pth, hash_kind):
    """The node len(pth) levels above leaf `leaf` (its position inside that sub-tree is leaf mod 2^len)."""
    leaf &= (1 << len(pth)) - 1
    if hash_kind == blake2s_ref.HASH_KIND:
        return blake2s_ref.root_from_leaf(slots, leaf, pth)
    return coset_ref.root_from_leaf(orc, slots, leaf, pth, hash_kind)


class Committed:
    """layers[id], trees[id] (whole heaps), lg[id], ce[id], caps[id] (the committed bytes) for the committed ids, betas[r0], alphas, coef
    (the free term alone when D = 0), and the channel after the free term / the coefficients."""


@functools.lru_cache(maxsize=32)
def committed(orc, log_n, log_b, hash_kind, K, coset, D, c, a1=3141592, prefix=b""):
    assert stop_ref.admissible(log_n, log_b, D) and 0 <= c <= MAX_CAP
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    Rp = log_n - D
    grp = groups(Rp, K)
    out = Committed()
    out.public_last, out.layers, out.trees, out.lg, out.ce, out.caps, out.betas = r.public_last, {}, {}, {}, {}, {}, {}
    ch = _Channel(prefix)
    if hash_kind != blake2s_ref.HASH_KIND:
        orc.set_hash(hash_kind)
    try:
        def commit_layer(i, vals, steps):
            out.layers[i] = np.array(vals, dtype=np.uint32)
            out.trees[i] = _tree(orc, out.layers[i], steps, hash_kind)
            out.lg[i] = (len(out.trees[i]) + 1).bit_length() - 2
            out.ce[i] = c_eff(c, out.lg[i])
            out.caps[i] = cap_of(out.trees[i], out.ce[i])
            ch.commit(out.caps[i])                          # ONE commit of 32 * 2^ce bytes

        commit_layer(0, r.f_eval, 0)
        out.alphas = [ch.get_u32() for _ in range(3)]
        commit_layer(1, orc.compose(r.f_eval, log_n, log_b, out.alphas, r.public_last), grp[0][1] if coset else 0)
        for j, (r0, steps) in enumerate(grp):
            beta = out.betas[r0] = ch.get_u32()
            nxt = fold_layer(orc, out.layers[1 + r0], log_n, log_b, r0, steps, beta)
            if D and j + 1 == len(grp):
                out.layers[1 + Rp] = np.array(nxt, dtype=np.uint32)   # the stopped layer: no tree
            else:
                commit_layer(1 + r0 + steps, nxt, grp[j + 1][1] if coset and j + 1 < len(grp) else 0)
    finally:
        orc.set_hash(0)
    assert [(i, out.lg[i]) for i in sorted(out.lg)] == trees(log_n, log_b, K, coset, D)
    if D:
        out.coef = stop_ref.final_coefficients(out.layers[1 + Rp], log_n, log_b, D)
    else:
        last = out.layers[1 + log_n]
        assert len(last) == 1 << log_b and len(set(int(v) for v in last)) == 1
        out.coef = [int(last[0])]
    ch.commit(b"".join(struct.pack("<I", v) for v in out.coef))
    out.prefix_state, out.prefix_data = ch.state, bytes(ch.data)
    return out


def proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits=0, a1=3141592, prefix=b""):
    """The proof of fibsq(1, a1) with caps of 2^c: .data (the prefix included), .state, .public_last, .nonce, .raws, .c (Committed),
    .coef, .landed ({tree id: set of cap entries some path lands in})."""
    cm = committed(orc, log_n, log_b, hash_kind, K, bool(coset), D, c, a1, prefix)
    L, N, B = log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = cm.prefix_state, bytearray(cm.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce, out.coef = cm, cm.public_last, None, list(cm.coef)
    out.landed = {i: set() for i in cm.trees}
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]

    def counted_path(tid, leaf):
        plen = cm.lg[tid] - cm.ce[tid]
        out.landed[tid].add(leaf >> plen)
        return struct.pack("<Q", plen) + b"".join(cut_path(cm.trees[tid], leaf, cm.ce[tid]))

    for raw in raws:
        x = raw % (N - 2 * B)
        for lid, idx in ((0, x), (0, x + B), (0, x + 2 * B)) + (() if coset else ((1, x),)):
            ch.commit(struct.pack("<I", int(cm.layers[lid][idx])) + counted_path(lid, idx))
        for r0, steps in groups(log_n - D, K):
            layer = cm.layers[1 + r0]
            if coset:
                m = (N >> r0) >> steps
                leaf = x % m
                ch.commit(b"".join(struct.pack("<I", int(layer[leaf + u * m])) for u in range(1 << steps)) + counted_path(1 + r0, leaf))
            else:
                s, size = 1 << steps, N >> r0
                idx = [(x % size + t * (size // s)) % size for t in range(s)]
                ch.commit(b"".join(struct.pack("<I", int(layer[i])) for i in idx) + b"".join(counted_path(1 + r0, i) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    assert len(out.data) - len(prefix) == proof_len(log_n, log_b, q, bits, K, coset, D, c)
    return out


def regions(log_n, log_b, q, bits, K, coset, D, c):
    """[(name, offset, length)] of every field in wire order.  The cap of a tree is one region per entry: f_root.e<i>, root<j>.e<i>."""
    L, grp, out, o = log_n + log_b, groups(log_n - D, K), [], 0
    lg = dict(trees(log_n, log_b, K, coset, D))

    def add(name, n):
        nonlocal o
        out.append((name, o, n))
        o += n

    def add_cap(name, tid):
        for i in range(1 << c_eff(c, lg[tid])):
            add(f"{name}.e{i}", 32)

    add_cap("f_root", 0)
    for i in range(3):
        add(f"alpha{i}", 4)
    add_cap("root0", 1)
    for j, (r0, steps) in enumerate(grp):
        add(f"beta{j}", 4)
        if not D or j + 1 < len(grp):
            add_cap(f"root{j + 1}", 1 + r0 + steps)
    if D:
        for k in range(1 << D):
            add(f"coef{k}", 4)
    else:
        add("free_term", 4)
    if bits:
        add("nonce", 8)
    for k in range(q):
        add(f"raw{k}", 4)
    for k in range(q):
        for i in range(3 if coset else 4):
            add(f"q{k}.f{i}.value", 4)
            add(f"q{k}.f{i}.count", 8)
            add(f"q{k}.f{i}.path", 32 * (L - c_eff(c, lg[0 if i < 3 else 1])))
        for j, (r0, steps) in enumerate(grp):
            plen = lg[1 + r0] - c_eff(c, lg[1 + r0])
            if coset:
                for u in range(1 << steps):
                    add(f"q{k}.g{j}.slot{u}", 4)
                add(f"q{k}.g{j}.count", 8)
                add(f"q{k}.g{j}.path", 32 * plen)
            else:
                for t in range(1 << steps):
                    add(f"q{k}.g{j}.value{t}", 4)
                for t in range(1 << steps):
                    add(f"q{k}.g{j}.count{t}", 8)
                    add(f"q{k}.g{j}.path{t}", 32 * plen)
    assert o == proof_len(log_n, log_b, q, bits, K, coset, D, c)
    return out


# ---- the verifier, in plain Python ---------------------------------------------------------------------------------------------
def _ok(log_n, log_b, q, bits, K, coset, D, c, n):
    return stop_ref.admissible(log_n, log_b, D) and 0 <= c <= MAX_CAP and n == proof_len(log_n, log_b, q, bits, K, coset, D, c)


def replay(data, state, log_n, log_b, q, bits, K, coset, D, c):
    """The Fiat-Shamir replay: 0, -1 (length or limits), -(1000 + k) for the k-th of the 3 + G + q challenges, -1998 for the nonce,
    -1999 for the state.  Each cap is one commit."""
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, len(data)):
        return -1
    L, grp = log_n + log_b, groups(log_n - D, K)
    lg = dict(trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    ch, rd, k = _Channel(), _Reader(data), 0

    def challenge():
        want = struct.unpack(">I", ch.state[:4])[0]
        b = rd.take(4)
        if struct.unpack("<I", b)[0] != want:
            return False
        ch.commit(b)
        return True

    ch.commit(rd.take(32 << ce[0]))
    for _ in range(3):
        k += 1
        if not challenge():
            return -(1000 + k)
    ch.commit(rd.take(32 << ce[1]))
    for j, (r0, steps) in enumerate(grp):
        k += 1
        if not challenge():
            return -(1000 + k)
        if not D or j + 1 < len(grp):
            ch.commit(rd.take(32 << ce[1 + r0 + steps]))
    ch.commit(rd.take(4 << D))                              # the free term, or the coefficients in one piece
    if bits:
        ch.commit(rd.take(8))
        if struct.unpack(">I", ch.state[:4])[0] >> (32 - bits):
            return -1998
    for _ in range(q):
        k += 1
        if not challenge():
            return -(1000 + k)
    for _ in range(q):
        for i in range(3 if coset else 4):
            ch.commit(rd.take(12 + 32 * (L - ce[0 if i < 3 else 1])))
        for r0, steps in grp:
            plen = lg[1 + r0] - ce[1 + r0]
            ch.commit(rd.take(4 * (1 << steps) + 8 + 32 * plen if coset else (1 << steps) * (12 + 32 * plen)))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c):
    """The check number of the CPU verifier (zk_verify_cap): strict (the replay first) when state is not None.  c = 0 hands over to
    blake2s_ref.verify, the model of the cap-free format for every hash."""
    if c == 0:
        return blake2s_ref.verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D)
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K, coset, D, c)
        if rc:
            return rc
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, len(data)):
        return -1                                           # a capped proof of another length is -1, strict or not
    if hash_kind != blake2s_ref.HASH_KIND:
        orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c)
    finally:
        orc.set_hash(0)


def _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c):
    n, L, Rp = 1 << log_n, log_n + log_b, log_n - D
    N, B = 1 << L, 1 << log_b
    grp = groups(Rp, K)
    G, nf = len(grp), 3 if coset else 4
    lg = dict(trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    rd = _Reader(data)
    try:
        f_cap = rd.take(32 << ce[0])
        alpha = [rd.u32() for _ in range(3)]
        caps = [rd.take(32 << ce[1])]                       # caps[j]: of the tree over group j's input layer
        betas = []
        for j, (r0, steps) in enumerate(grp):
            betas.append(rd.u32())
            if not D or j + 1 < G:
                caps.append(rd.take(32 << ce[1 + r0 + steps]))
        coef = [rd.u32() for _ in range(1 << D)]            # D = 0: the free term, compared unreduced
        if bits:
            rd.take(8)
        raws = [rd.u32() for _ in range(q)]
    except _Short:
        return -1

    def misses(slots, leaf, pth, cap):                      # the path must land on entry leaf >> len(path) of the cap
        e = leaf >> len(pth)
        return _climb(orc, slots, leaf, pth, hash_kind) != cap[32 * e:32 * e + 32]

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
        if any(len(fp[i]) != L - ce[0 if i < 3 else 1] for i in range(nf)):
            return -3
        for i, (idx, cap) in enumerate(((tp, f_cap), (tp + B, f_cap), (tp + 2 * B, f_cap), (tp, caps[0]))[:nf]):
            if misses([fv[i]], idx, fp[i], cap):
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
            plen = lg[1 + r0] - ce[1 + r0]
            if coset:
                m = size >> steps
                if len(lp[j][0]) != plen:
                    return -(200 + j)
                if misses(lv[j], tp % m, lp[j][0], caps[j]):
                    return -(300 + j)
                continue
            if any(len(p) != plen for p in lp[j]):
                return -(200 + j)
            for t in range(s):
                if misses([lv[j][t]], (tp % size + t * (size // s)) % size, lp[j][t], caps[j]):
                    return -(300 + j) if t == 0 else -(400 + j)
    return -8 if rd.p != len(data) else 0
