"""Shared proofs with row leaves (zk_batch_set_shared_rows, zk_verify_shared_rows) built without the library, and a
plain-Python verifier of that format (tests/test_shared_rows.py, tests/test_gpu_shared_rows.py).

The M = 2^lb trace polynomials of a shared proof (tests/shared_ref.py) are committed as ONE tree over N leaves, leaf i holding the row
(f_0[i], .., f_{M-1}[i]): the header opens with that tree's cap (2^ce_f digests, one commit), the 3M alphas and everything from cp on are
shared_ref's, and a query opens three rows -- M values, a count, ONE path each -- in place of 3M f tuples.  The challenges follow the
commitments, so the transcript is walked again here with the primitives of shared_ref / cap_ref / fold_ref, which stay as they are.  What
this module hashes itself is the row leaf: hashlib.sha256, and the field chain over orc.fieldhash_permute the way coset_ref.leaf_hash
does one compression."""
import functools
import hashlib
import struct

import numpy as np

import cap_ref
import grind_ref
import shared_ref
import stop_ref
from cap_ref import c_eff, cap_of, cut_path
from fold_ref import GEN_W, P, RefProof, _Channel, _inv, _Reader, _Short, fold_layer, groups

MAX_LB = shared_ref.MAX_LB
SEED = shared_ref.SEED


def _compress(orc, words):
    """The field hash's compression of 16 words: the first 8 of permute(words) + words."""
    state = [int(v) % P for v in words]
    out = orc.fieldhash_permute(np.array(state, dtype=np.uint32))
    return [(int(out[i]) + state[i]) % P for i in range(8)]


def row_leaf_hash(orc, values, hash_kind):
    """The digest of a row of M = len(values) values, M a power of two <= 256.  SHA-256: of the 4M bytes, big-endian per value.  Field
    hash: M <= 8 the coset leaf (v, 0.., M); M >= 16 the chain c_0 = compress(v_0..v_7, 0.., M), c_k = compress(c_{k-1} || v_8k..v_8k+7)."""
    m = len(values)
    assert m & (m - 1) == 0 and 1 <= m <= 256
    if hash_kind == 0:
        return hashlib.sha256(b"".join(struct.pack(">I", int(v)) for v in values)).digest()
    assert hash_kind == 1
    first = [int(v) for v in values[:8]]
    c = _compress(orc, first + [0] * (15 - len(first)) + [m])
    for k in range(1, m // 8):
        c = _compress(orc, c + [int(v) for v in values[8 * k:8 * k + 8]])
    return b"".join(struct.pack(">I", w) for w in c)


def rows_tree(orc, f, hash_kind):
    """Heap ([2N - 1, 32] uint8) of the tree over the rows of f ([M][N]); orc.set_hash(hash_kind) is in force for the inner nodes."""
    M, N = len(f), len(f[0])
    heap = [None] * (2 * N - 1)
    for i in range(N):
        heap[N - 1 + i] = row_leaf_hash(orc, [f[p][i] for p in range(M)], hash_kind)
    for i in range(N - 2, -1, -1):
        heap[i] = orc.node_hash(heap[2 * i + 1], heap[2 * i + 2])
    return np.frombuffer(b"".join(heap), dtype=np.uint8).reshape(2 * N - 1, 32)


def _climb(orc, values, leaf, pth, hash_kind):
    """The node len(pth) levels above row leaf `leaf`; orc.set_hash(hash_kind) is in force."""
    cur, i = row_leaf_hash(orc, values, hash_kind), (leaf & ((1 << len(pth)) - 1)) + (1 << len(pth)) - 1
    for sib in pth:
        cur = orc.node_hash(cur, sib) if i & 1 else orc.node_hash(sib, cur)
        i = (i - 1) >> 1
    return cur


def proof_len(log_n, log_b, q, bits, K, coset, D, c, lb):
    """The issue's formula: a single proof's length plus 12 (M - 1) (1 + q) -- the further alphas, and 4 (M - 1) more value bytes in each
    of the 3 q row tuples."""
    return cap_ref.proof_len(log_n, log_b, q, bits, K, coset, D, c) + 12 * ((1 << lb) - 1) * (1 + q)


class Committed:
    """f[p], last[p] per statement, f_tree (the heap over the rows), and shared_ref.Committed's fields for the one FRI."""


@functools.lru_cache(maxsize=16)
def committed(orc, log_n, log_b, lb, hash_kind, K, coset, D, c, first=SEED):
    assert stop_ref.admissible(log_n, log_b, D) and 0 <= c <= cap_ref.MAX_CAP and 1 <= lb <= MAX_LB and hash_kind in (0, 1)
    M, L, Rp = 1 << lb, log_n + log_b, log_n - D
    grp = groups(Rp, K)
    out = Committed()
    out.f, out.last = [], []
    out.layers, out.trees, out.lg, out.ce, out.caps, out.betas = {}, {}, {}, {}, {}, {}
    for p in range(M):
        r = orc.prove(log_n, log_b, 1, first + p, want_vectors=True)
        assert r.rc == 0
        out.f.append(np.array(r.f_eval, dtype=np.uint32))
        out.last.append(int(r.public_last))
    ch = _Channel()
    orc.set_hash(hash_kind)
    try:
        out.ce[0] = c_eff(c, L)
        out.f_tree = rows_tree(orc, out.f, hash_kind)
        ch.commit(cap_of(out.f_tree, out.ce[0]))              # the cap of the ONE tree over the rows: one commit
        out.alphas = [ch.get_u32() for _ in range(3 * M)]
        cp = np.zeros(1 << L, dtype=np.uint64)
        for p in range(M):
            cp = (cp + np.array(orc.compose(out.f[p], log_n, log_b, out.alphas[3 * p:3 * p + 3], out.last[p]), dtype=np.uint64)) % P

        def commit_layer(i, vals, steps):
            out.layers[i] = np.array(vals, dtype=np.uint32)
            out.trees[i] = cap_ref._tree(orc, out.layers[i], steps, hash_kind)
            out.lg[i] = (len(out.trees[i]) + 1).bit_length() - 2
            out.ce[i] = c_eff(c, out.lg[i])
            out.caps[i] = cap_of(out.trees[i], out.ce[i])
            ch.commit(out.caps[i])

        commit_layer(1, cp, grp[0][1] if coset else 0)
        for j, (r0, steps) in enumerate(grp):
            beta = out.betas[r0] = ch.get_u32()
            nxt = fold_layer(orc, out.layers[1 + r0], log_n, log_b, r0, steps, beta)
            if D and j + 1 == len(grp):
                out.layers[1 + Rp] = np.array(nxt, dtype=np.uint32)
            else:
                commit_layer(1 + r0 + steps, nxt, grp[j + 1][1] if coset and j + 1 < len(grp) else 0)
    finally:
        orc.set_hash(0)
    assert [(i, out.lg[i]) for i in sorted(out.lg)] == cap_ref.trees(log_n, log_b, K, coset, D)[1:]
    if D:
        out.coef = stop_ref.final_coefficients(out.layers[1 + Rp], log_n, log_b, D)
    else:
        last = out.layers[1 + log_n]
        assert len(last) == 1 << log_b and len(set(int(v) for v in last)) == 1
        out.coef = [int(last[0])]
    ch.commit(b"".join(struct.pack("<I", v) for v in out.coef))
    out.prefix_state, out.prefix_data = ch.state, bytes(ch.data)
    return out


def proof(orc, log_n, log_b, lb, q, hash_kind, K, coset, D, c, bits=0, first=SEED):
    """The shared proof with row leaves of fibsq(1, first + p), p < 2^lb: .data, .state, .public_last (list), .nonce, .raws, .c."""
    cm = committed(orc, log_n, log_b, lb, hash_kind, K, bool(coset), D, c, first)
    M, L, N, B = 1 << lb, log_n + log_b, 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = cm.prefix_state, bytearray(cm.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce, out.coef = cm, list(cm.last), None, list(cm.coef)
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]

    def path(tree, lg, ce, leaf):
        return struct.pack("<Q", lg - ce) + b"".join(cut_path(tree, leaf, ce))

    for raw in raws:
        x = raw % (N - 2 * B)
        for idx in (x, x + B, x + 2 * B):                      # a row: M values in statement order, one count, one path
            ch.commit(b"".join(struct.pack("<I", int(cm.f[p][idx])) for p in range(M)) + path(cm.f_tree, L, cm.ce[0], idx))
        if not coset:
            ch.commit(struct.pack("<I", int(cm.layers[1][x])) + path(cm.trees[1], cm.lg[1], cm.ce[1], x))
        for r0, steps in groups(log_n - D, K):
            layer, tid = cm.layers[1 + r0], 1 + r0
            if coset:
                m = (N >> r0) >> steps
                leaf = x % m
                ch.commit(b"".join(struct.pack("<I", int(layer[leaf + u * m])) for u in range(1 << steps)) + path(cm.trees[tid], cm.lg[tid], cm.ce[tid], leaf))
            else:
                s, size = 1 << steps, N >> r0
                idx = [(x % size + t * (size // s)) % size for t in range(s)]
                ch.commit(b"".join(struct.pack("<I", int(layer[i])) for i in idx) + b"".join(path(cm.trees[tid], cm.lg[tid], cm.ce[tid], i) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    assert len(out.data) == proof_len(log_n, log_b, q, bits, K, coset, D, c, lb)
    return out


def regions(log_n, log_b, q, bits, K, coset, D, c, lb):
    """[(name, offset, length)] of every field in wire order: f_root.e<i>, s<p>.alpha<i>, then cap_ref's names from root0 on, and per query
    q<k>.row<i>.value<p> (M of them), q<k>.row<i>.count, q<k>.row<i>.path in front of cap_ref's cp and group fields."""
    M, L = 1 << lb, log_n + log_b
    ce_f = c_eff(c, L)
    out, o = [], 0

    def add(name, n):
        nonlocal o
        out.append((name, o, n))
        o += n

    for i in range(1 << ce_f):
        add(f"f_root.e{i}", 32)
    for p in range(M):
        for i in range(3):
            add(f"s{p}.alpha{i}", 4)
    single = cap_ref.regions(log_n, log_b, q, bits, K, coset, D, c)
    for name, _, n in single:
        if not name.startswith("q") and not name.startswith("f_root") and not name.startswith("alpha"):
            add(name, n)
    for k in range(q):
        for i in range(3):
            for p in range(M):
                add(f"q{k}.row{i}.value{p}", 4)
            add(f"q{k}.row{i}.count", 8)
            add(f"q{k}.row{i}.path", 32 * (L - ce_f))
        for name, _, n in single:
            if name.startswith(f"q{k}.") and not any(name.startswith(f"q{k}.f{i}.") for i in range(3)):
                add(name, n)
    assert o == proof_len(log_n, log_b, q, bits, K, coset, D, c, lb)
    return out


# ---- the verifier, in plain Python ---------------------------------------------------------------------------------------------
def _ok(log_n, log_b, q, bits, K, coset, D, c, lb, hash_kind, n):
    return (stop_ref.admissible(log_n, log_b, D) and 0 <= c <= cap_ref.MAX_CAP and 1 <= lb <= MAX_LB and hash_kind in (0, 1) and
            n == proof_len(log_n, log_b, q, bits, K, coset, D, c, lb))


def replay(data, state, log_n, log_b, q, bits, K, coset, D, c, lb):
    """The Fiat-Shamir replay: 0, -1, -(1000 + k) for the k-th of the 3M + G + q challenges, -1998 for the nonce, -1999 for the state.
    The f cap is one commit, each row tuple one commit."""
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, lb, 0, len(data)):
        return -1
    M, L, grp = 1 << lb, log_n + log_b, groups(log_n - D, K)
    lg = dict(cap_ref.trees(log_n, log_b, K, coset, D))
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
    for _ in range(3 * M):
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
    ch.commit(rd.take(4 << D))
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
            ch.commit(rd.take(4 * M + 8 + 32 * (L - ce[0])))
        if not coset:
            ch.commit(rd.take(12 + 32 * (L - ce[1])))
        for r0, steps in grp:
            plen = lg[1 + r0] - ce[1 + r0]
            ch.commit(rd.take(4 * (1 << steps) + 8 + 32 * plen if coset else (1 << steps) * (12 + 32 * plen)))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, lb, hash_kind, q, bits, K, coset, D, c):
    """The check number of zk_verify_shared_rows(.., 1, ..): strict (the replay first) when state is not None."""
    if not 1 <= lb <= MAX_LB or hash_kind not in (0, 1):
        return -1
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K, coset, D, c, lb)
        if rc:
            return rc
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, lb, hash_kind, len(data)):
        return -1
    orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, lb, hash_kind, q, bits, K, coset, D, c)
    finally:
        orc.set_hash(0)


def _verify(orc, data, log_n, log_b, public_last, lb, hash_kind, q, bits, K, coset, D, c):
    M, n, L, Rp = 1 << lb, 1 << log_n, log_n + log_b, log_n - D
    N, B = 1 << L, 1 << log_b
    grp = groups(Rp, K)
    G = len(grp)
    lg = dict(cap_ref.trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    rd = _Reader(data)
    try:
        f_cap = rd.take(32 << ce[0])
        alpha = [rd.u32() for _ in range(3 * M)]
        caps = [rd.take(32 << ce[1])]
        betas = []
        for j, (r0, steps) in enumerate(grp):
            betas.append(rd.u32())
            if not D or j + 1 < G:
                caps.append(rd.take(32 << ce[1 + r0 + steps]))
        coef = [rd.u32() for _ in range(1 << D)]
        if bits:
            rd.take(8)
        raws = [rd.u32() for _ in range(q)]
    except _Short:
        return -1

    def misses(slots, leaf, pth, cap):
        e = leaf >> len(pth)
        return cap_ref._climb(orc, slots, leaf, pth, hash_kind) != cap[32 * e:32 * e + 32]

    g, h = pow(GEN_W, (P - 1) >> log_n, P), pow(GEN_W, (P - 1) >> L, P)
    inv2 = _inv(2)
    for raw in raws:
        try:
            rows, rp = [], []
            for _ in range(3):
                rows.append([rd.u32() for _ in range(M)])
                rp.append(rd.path())
            cpv = cpp = None
            if not coset:
                cpv, cpp = rd.u32(), rd.path()
            lv, lp = [], []
            for r0, steps in grp:
                lv.append([rd.u32() for _ in range(1 << steps)])
                lp.append([rd.path() for _ in range(1 if coset else 1 << steps)])
        except _Short:
            return -1
        tp = raw % (N - 2 * B)

        def val(j, t):
            if not coset:
                return lv[j][t]
            r0, steps = grp[j]
            size, s = N >> r0, 1 << steps
            return lv[j][((tp % size) // (size // s) + t) % s]

        x = GEN_W * pow(h, tp, P) % P
        gm1 = _inv(g)
        gm2, gm3 = gm1 * gm1 % P, gm1 * gm1 * gm1 % P
        den = (pow(x, n, P) - 1) * _inv((x - gm3) * (x - gm2) * (x - gm1) % P) % P
        total = 0
        for p in range(M):
            f_x, f_gx, f_ggx = rows[0][p] % P, rows[1][p] % P, rows[2][p] % P
            p0 = (f_x - 1) * _inv((x - 1) % P) % P
            p1 = (f_x - public_last[p] % P) * _inv((x - gm2) % P) % P
            p2 = (f_ggx - f_gx * f_gx - f_x * f_x) % P * _inv(den) % P
            total = (total + alpha[3 * p] % P * p0 + alpha[3 * p + 1] % P * p1 + alpha[3 * p + 2] % P * p2) % P
        if total != (val(0, 0) if coset else cpv):
            return -2
        if any(len(p) != L - ce[0] for p in rp) or (not coset and len(cpp) != L - ce[1]):
            return -3
        for i, idx in enumerate((tp, tp + B, tp + 2 * B)):
            if _climb(orc, rows[i], idx, rp[i], hash_kind) != f_cap[32 * (idx >> len(rp[i])):32 * (idx >> len(rp[i])) + 32]:
                return -(4 + i)
        if not coset and misses([cpv], tp, cpp, caps[0]):
            return -7
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
            else:
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
