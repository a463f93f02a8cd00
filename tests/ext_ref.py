"""The quadratic extension E = F_P[u] / (u^2 - 5) and the two prover stages that run over it, built without the library
(tests/test_ext_field.py, tests/test_gpu_ext_kernels.py), and proofs of the ext_log = 1 format with a plain-Python verifier of it
(tests/test_ext_verify.py, tests/test_host_sanitizers_ext.py); DESIGN.md 7j.

E arithmetic in Python integers; the components of cp from the oracle's base-field composition with the component alphas (cp is
linear in the alphas and the quotients stay in the base field); the fold written out in numpy from its definition
    next(x^2) = (v(x) + v(-x)) / 2 + beta (v(x) - v(-x)) / (2 x),   v and beta in E, x in the base field,
on a layer of two planes (component 0 at [0, len), component 1 at [len, 2 len))."""
import functools
import struct

import numpy as np

import cap_ref
import coset_ref
import grind_ref
import rows_ref
import stop_ref
from cap_ref import c_eff, cap_of, cut_path
from fold_ref import RefProof, _Channel, _inv, _Reader, _Short, groups

P = 3221225473
GEN_W = 5
NONRESIDUE = 5          # u^2
SHIFT = 5               # the coset shift of every domain the tests build


def reduce(a):
    return (a[0] % P, a[1] % P)


def mul(a, b):
    (a0, a1), (b0, b1) = reduce(a), reduce(b)
    return ((a0 * b0 + NONRESIDUE * a1 * b1) % P, (a0 * b1 + a1 * b0) % P)


def inv(a):
    a0, a1 = reduce(a)
    norm = (a0 * a0 - NONRESIDUE * a1 * a1) % P
    if norm == 0:
        raise ZeroDivisionError("the inverse of zero in E")          # the norm of a non-zero element is non-zero: 5 is a non-residue
    ni = pow(norm, P - 2, P)
    return (a0 * ni % P, (P - a1) % P * ni % P)


def power(a, e):
    r, b = (1, 0), reduce(a)
    while e:
        if e & 1:
            r = mul(r, b)
        b = mul(b, b)
        e >>= 1
    return r


def compose_planes(orc, f_eval, log_n, log_b, alpha_raw6, public_last):
    """cp over E as two planes: alpha_raw6 = alpha0.c0, alpha0.c1, alpha1.c0, alpha1.c1, alpha2.c0, alpha2.c1 (the order of the draws)."""
    return np.concatenate([orc.compose(f_eval, log_n, log_b, [alpha_raw6[j], alpha_raw6[2 + j], alpha_raw6[4 + j]], public_last) for j in (0, 1)])


def _mulmod(a, b):
    """a * b mod P for an array a and an integer or an array b, all below 2^32 (the product fits 64 bits)."""
    b = np.uint64(b % P) if isinstance(b, int) else b.astype(np.uint64)
    return a.astype(np.uint64) * b % np.uint64(P)


def _powers(g, count):
    """g^0 .. g^(count-1) mod P, count a power of two, by doubling."""
    out = np.ones(1, dtype=np.uint64)
    while len(out) < count:
        out = np.concatenate([out, _mulmod(out, pow(g, len(out), P))])
    return out


def fold_once(planes, log_n, log_b, rnd, beta):
    """One round: the layer of round `rnd` (2^(L - rnd) values of E at (SHIFT h^i)^(2^rnd)) -> round rnd + 1; beta = (b0, b1) reduced."""
    L = log_n + log_b
    m = 1 << (L - rnd)
    half = m // 2
    planes = np.asarray(planes, dtype=np.uint64)
    assert len(planes) == 2 * m
    h = pow(GEN_W, (P - 1) >> L, P)
    x0_inv = pow(pow(SHIFT, 1 << rnd, P), P - 2, P)
    hr_inv = pow(pow(h, 1 << rnd, P), P - 2, P)
    inv2 = pow(2, P - 2, P)
    inv_2x = _mulmod(_powers(hr_inv, half), x0_inv * inv2 % P)          # 1 / (2 x_i), i < half
    s, d = [], []
    for j in (0, 1):
        v = planes[j * m:(j + 1) * m]
        lo, hi = v[:half], v[half:]                                        # v(x_i), v(-x_i): x_(i + half) = -x_i
        s.append(_mulmod((lo + hi) % np.uint64(P), inv2))
        d.append(_mulmod((lo + np.uint64(P) - hi) % np.uint64(P), inv_2x))
    b0, b1 = beta
    c0 = (s[0] + _mulmod(d[0], b0) + _mulmod(_mulmod(d[1], b1), NONRESIDUE)) % np.uint64(P)
    c1 = (s[1] + _mulmod(d[0], b1) + _mulmod(d[1], b0)) % np.uint64(P)
    return np.concatenate([c0, c1]).astype(np.uint32)


def fold_layer(planes, log_n, log_b, r0, steps, beta_raw2):
    """A group of `steps` rounds from round r0 with the challenges beta, beta^2, beta^4, the squares taken in E."""
    b = reduce(beta_raw2)
    for t in range(steps):
        planes = fold_once(planes, log_n, log_b, r0 + t, b)
        b = mul(b, b)
    return planes


# ---- proofs of the ext_log = 1 format, built without the library ------------------------------------------------------------------
# The format is the one of csrc/transcript.hpp ("ext"): the walk of cap_ref with challenges, cp and the FRI layers in E.  The
# oracle gives the trace and f; cp is compose_planes, the folds are fold_layer above, the leaves of every tree over a layer of E are
# rows_ref.row_leaf_hash of the leaf's 2 S words, inner nodes are the oracle's, caps and cut paths are cap_ref's, the final coefficients are
# stop_ref.final_coefficients of each plane.


def trees(log_n, log_b, K, coset, D):
    """[(tree id, lg)] in commit order, as cap_ref.trees: the last tree (D = 0) has one value of E -- two words -- per leaf."""
    return cap_ref.trees(log_n, log_b, K, coset, D)


def proof_len(log_n, log_b, q, bits, K, coset, D, c):
    """Written out from the definition, not from the base-field lengths."""
    L, grp = log_n + log_b, groups(log_n - D, K)
    lg = dict(trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    head = (32 << ce[0]) + 24 + (32 << ce[1])
    for j, (r0, steps) in enumerate(grp):
        head += 8 + ((32 << ce[1 + r0 + steps]) if (not D or j + 1 < len(grp)) else 0)
    head += (8 << D) + (8 if bits else 0) + 4 * q
    per_query = 3 * (4 + 8 + 32 * (L - ce[0]))
    if not coset:
        per_query += 8 + 8 + 32 * (L - ce[1])
    for r0, steps in grp:
        plen = lg[1 + r0] - ce[1 + r0]
        per_query += (8 << steps) + 8 + 32 * plen if coset else (1 << steps) * (8 + 8 + 32 * plen)
    return head + q * per_query


def leaf_words(planes, steps, leaf):
    """The 2 S words of leaf `leaf` of the tree with 2^steps slots per leaf: the S component-0 words in slot order, then the S component-1 words."""
    ln = len(planes) // 2
    m = ln >> steps
    return [int(planes[j * ln + leaf + u * m]) for j in (0, 1) for u in range(1 << steps)]


def tree(orc, planes, steps, hash_kind):
    """Heap [2 m - 1, 32] over a layer of E; orc.set_hash(hash_kind) is in force for the inner nodes."""
    m = (len(planes) // 2) >> steps
    heap = [None] * (2 * m - 1)
    for leaf in range(m):
        heap[m - 1 + leaf] = rows_ref.row_leaf_hash(orc, leaf_words(planes, steps, leaf), hash_kind)
    for i in range(m - 2, -1, -1):
        heap[i] = orc.node_hash(heap[2 * i + 1], heap[2 * i + 2])
    return np.frombuffer(b"".join(heap), dtype=np.uint8).reshape(2 * m - 1, 32)


class Committed:
    """layers[id] (id 0: f; id >= 1: two planes), trees[id], lg[id], ce[id], caps[id], alphas (6 raws), betas[r0] = (c0, c1) raws, coef (the
    words of kFinal in wire order), and the channel after them."""


@functools.lru_cache(maxsize=64)
def committed(orc, log_n, log_b, hash_kind, K, coset, D, c, a1=3141592, prefix=b""):
    """prefix: what the channel holds before the proof starts (zk_prove_channel), as cap_ref.committed."""
    assert stop_ref.admissible(log_n, log_b, D) and 0 <= c <= cap_ref.MAX_CAP and hash_kind in (0, 1)
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    Rp = log_n - D
    grp = groups(Rp, K)
    out = Committed()
    out.public_last, out.layers, out.trees, out.lg, out.ce, out.caps, out.betas = r.public_last, {}, {}, {}, {}, {}, {}
    ch = _Channel(prefix)
    orc.set_hash(hash_kind)
    try:
        def commit_tree(i, heap):
            out.trees[i] = heap
            out.lg[i] = (len(heap) + 1).bit_length() - 2
            out.ce[i] = c_eff(c, out.lg[i])
            out.caps[i] = cap_of(heap, out.ce[i])
            ch.commit(out.caps[i])

        def commit_layer(i, planes, steps):
            out.layers[i] = np.array(planes, dtype=np.uint32)
            commit_tree(i, tree(orc, out.layers[i], steps, hash_kind))

        out.layers[0] = np.array(r.f_eval, dtype=np.uint32)
        commit_tree(0, orc.merkle_build(out.layers[0]))
        out.alphas = [ch.get_u32() for _ in range(6)]           # alpha0.c0, alpha0.c1, alpha1.c0, ..
        commit_layer(1, compose_planes(orc, r.f_eval, log_n, log_b, out.alphas, r.public_last), grp[0][1] if coset else 0)
        for j, (r0, steps) in enumerate(grp):
            beta = out.betas[r0] = (ch.get_u32(), ch.get_u32())
            nxt = fold_layer(out.layers[1 + r0], log_n, log_b, r0, steps, beta)
            if D and j + 1 == len(grp):
                out.layers[1 + Rp] = np.array(nxt, dtype=np.uint32)
            else:
                commit_layer(1 + r0 + steps, nxt, grp[j + 1][1] if coset and j + 1 < len(grp) else 0)
    finally:
        orc.set_hash(0)
    assert [(i, out.lg[i]) for i in sorted(out.lg)] == trees(log_n, log_b, K, coset, D)
    last = out.layers[1 + Rp]
    half = len(last) // 2
    if D:
        out.coef = [v for j in (0, 1) for v in stop_ref.final_coefficients(last[j * half:(j + 1) * half], log_n, log_b, D)]
    else:
        assert half == 1 << log_b and all(len(set(int(v) for v in last[j * half:(j + 1) * half])) == 1 for j in (0, 1))   # both planes constant
        out.coef = [int(last[0]), int(last[half])]
    ch.commit(b"".join(struct.pack("<I", v) for v in out.coef))
    out.prefix_state, out.prefix_data = ch.state, bytes(ch.data)
    return out


def proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits=0, a1=3141592, prefix=b""):
    """.data (the prefix included), .state, .public_last, .nonce, .raws, .c (Committed)."""
    cm = committed(orc, log_n, log_b, hash_kind, K, bool(coset), D, c, a1, prefix)
    N, B = 1 << (log_n + log_b), 1 << log_b
    ch = _Channel()
    ch.state, ch.data = cm.prefix_state, bytearray(cm.prefix_data)
    out = RefProof()
    out.c, out.public_last, out.nonce = cm, cm.public_last, None
    if bits:
        out.nonce = grind_ref.smallest_nonce(ch.state, bits)
        ch.commit(struct.pack("<Q", out.nonce))
    raws = [ch.get_u32() for _ in range(q)]

    def counted_path(tid, leaf):
        return struct.pack("<Q", cm.lg[tid] - cm.ce[tid]) + b"".join(cut_path(cm.trees[tid], leaf, cm.ce[tid]))

    def words(ws):
        return b"".join(struct.pack("<I", w) for w in ws)

    for raw in raws:
        x = raw % (N - 2 * B)
        for idx in (x, x + B, x + 2 * B):
            ch.commit(struct.pack("<I", int(cm.layers[0][idx])) + counted_path(0, idx))
        if not coset:
            ch.commit(words(leaf_words(cm.layers[1], 0, x)) + counted_path(1, x))
        for r0, steps in groups(log_n - D, K):
            planes, size = cm.layers[1 + r0], N >> r0
            if coset:
                leaf = x % (size >> steps)
                ch.commit(words(leaf_words(planes, steps, leaf)) + counted_path(1 + r0, leaf))
            else:
                idx = [(x % size + t * (size >> steps)) % size for t in range(1 << steps)]
                ch.commit(words([int(planes[j * size + i]) for j in (0, 1) for i in idx]) + b"".join(counted_path(1 + r0, i) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    assert len(out.data) - len(prefix) == proof_len(log_n, log_b, q, bits, K, coset, D, c)
    return out


def regions(log_n, log_b, q, bits, K, coset, D, c):
    """[(name, offset, length)] of every field in wire order; the words of a value of E are regions of their own (.c0 / .c1)."""
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
        add(f"alpha{i}.c0", 4)
        add(f"alpha{i}.c1", 4)
    add_cap("root0", 1)
    for j, (r0, steps) in enumerate(grp):
        add(f"beta{j}.c0", 4)
        add(f"beta{j}.c1", 4)
        if not D or j + 1 < len(grp):
            add_cap(f"root{j + 1}", 1 + r0 + steps)
    for comp in (0, 1):
        for k in range(1 << D):
            add(f"coef{k}.c{comp}" if D else f"free_term.c{comp}", 4)
    if bits:
        add("nonce", 8)
    for k in range(q):
        add(f"raw{k}", 4)
    for k in range(q):
        for i in range(3):
            add(f"q{k}.f{i}.value", 4)
            add(f"q{k}.f{i}.count", 8)
            add(f"q{k}.f{i}.path", 32 * (L - c_eff(c, lg[0])))
        if not coset:
            add(f"q{k}.cp.c0", 4)
            add(f"q{k}.cp.c1", 4)
            add(f"q{k}.cp.count", 8)
            add(f"q{k}.cp.path", 32 * (L - c_eff(c, lg[1])))
        for j, (r0, steps) in enumerate(grp):
            plen = lg[1 + r0] - c_eff(c, lg[1 + r0])
            for comp in (0, 1):
                for t in range(1 << steps):
                    add(f"q{k}.g{j}.{'slot' if coset else 'value'}{t}.c{comp}", 4)
            for t in range(1 if coset else 1 << steps):
                add(f"q{k}.g{j}.count{t}", 8)
                add(f"q{k}.g{j}.path{t}", 32 * plen)
    assert o == proof_len(log_n, log_b, q, bits, K, coset, D, c)
    return out


# ---- the verifier, in plain Python -------------------------------------------------------------------------------------------------
def _ok(log_n, log_b, q, bits, K, coset, D, c, n):
    return stop_ref.admissible(log_n, log_b, D) and 0 <= c <= cap_ref.MAX_CAP and n == proof_len(log_n, log_b, q, bits, K, coset, D, c)


def replay(data, state, log_n, log_b, q, bits, K, coset, D, c):
    """0, -1, -(1000 + k) for the k-th of the 6 + 2G + q challenges, -1998 for the nonce, -1999 for the state."""
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, len(data)):
        return -1
    L, grp = log_n + log_b, groups(log_n - D, K)
    lg = dict(trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    ch, rd, k = _Channel(), _Reader(data), 0

    def challenges(count):
        nonlocal k
        for _ in range(count):
            k += 1
            b = rd.take(4)
            if struct.unpack("<I", b)[0] != struct.unpack(">I", ch.state[:4])[0]:
                return False
            ch.commit(b)
        return True

    ch.commit(rd.take(32 << ce[0]))
    if not challenges(6):
        return -(1000 + k)
    ch.commit(rd.take(32 << ce[1]))
    for j, (r0, steps) in enumerate(grp):
        if not challenges(2):
            return -(1000 + k)
        if not D or j + 1 < len(grp):
            ch.commit(rd.take(32 << ce[1 + r0 + steps]))
    ch.commit(rd.take(8 << D))
    if bits:
        ch.commit(rd.take(8))
        if struct.unpack(">I", ch.state[:4])[0] >> (32 - bits):
            return -1998
    if not challenges(q):
        return -(1000 + k)
    for _ in range(q):
        for _ in range(3):
            ch.commit(rd.take(12 + 32 * (L - ce[0])))
        if not coset:
            ch.commit(rd.take(16 + 32 * (L - ce[1])))
        for r0, steps in grp:
            plen = lg[1 + r0] - ce[1 + r0]
            ch.commit(rd.take((8 << steps) + 8 + 32 * plen if coset else (1 << steps) * (16 + 32 * plen)))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c):
    """The check number zk_verify_ext must give with ext_log = 1: strict (the replay first) when state is not None."""
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K, coset, D, c)
        if rc:
            return rc
    if not _ok(log_n, log_b, q, bits, K, coset, D, c, len(data)):
        return -1
    orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c)
    finally:
        orc.set_hash(0)


def _climb(orc, leaf_ws, leaf, pth, hash_kind):
    cur, i = rows_ref.row_leaf_hash(orc, leaf_ws, hash_kind), (leaf & ((1 << len(pth)) - 1)) + (1 << len(pth)) - 1
    for sib in pth:
        cur = orc.node_hash(cur, sib) if i & 1 else orc.node_hash(sib, cur)
        i = (i - 1) >> 1
    return cur


def _verify(orc, data, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c):
    n, L, Rp = 1 << log_n, log_n + log_b, log_n - D
    N, B = 1 << L, 1 << log_b
    grp = groups(Rp, K)
    G = len(grp)
    lg = dict(trees(log_n, log_b, K, coset, D))
    ce = {t: c_eff(c, lg[t]) for t in lg}
    rd = _Reader(data)
    try:
        f_cap = rd.take(32 << ce[0])
        alpha = [rd.u32() for _ in range(6)]
        caps = [rd.take(32 << ce[1])]
        betas = []
        for j, (r0, steps) in enumerate(grp):
            betas.append((rd.u32(), rd.u32()))
            if not D or j + 1 < G:
                caps.append(rd.take(32 << ce[1 + r0 + steps]))
        coef = [rd.u32() for _ in range(2 << D)]
        if bits:
            rd.take(8)
        raws = [rd.u32() for _ in range(q)]
    except _Short:
        return -1

    def misses(ws, leaf, pth, cap):
        e = leaf >> len(pth)
        return _climb(orc, ws, leaf, pth, hash_kind) != cap[32 * e:32 * e + 32]

    def f_misses(v, leaf, pth):
        e = leaf >> len(pth)
        return coset_ref.root_from_leaf(orc, [v], leaf & ((1 << len(pth)) - 1), pth, hash_kind) != f_cap[32 * e:32 * e + 32]

    g, h = pow(GEN_W, (P - 1) >> log_n, P), pow(GEN_W, (P - 1) >> L, P)
    inv2 = _inv(2)
    for raw in raws:
        try:
            fv, fp = [], []
            for _ in range(3):
                fv.append(rd.u32())
                fp.append(rd.path())
            if not coset:
                cpw = [rd.u32(), rd.u32()]
                cpp = rd.path()
            lw, lp = [], []
            for r0, steps in grp:
                lw.append([rd.u32() for _ in range(2 << steps)])
                lp.append([rd.path() for _ in range(1 if coset else 1 << steps)])
        except _Short:
            return -1
        tp = raw % (N - 2 * B)

        def val(j, t):                                      # value t of group j, unreduced
            r0, steps = grp[j]
            size, s = N >> r0, 1 << steps
            u = ((tp % size) // (size // s) + t) % s if coset else t
            return (lw[j][u], lw[j][s + u])

        x = GEN_W * pow(h, tp, P) % P
        f_x, f_gx, f_ggx = fv[0] % P, fv[1] % P, fv[2] % P
        gm1 = _inv(g)
        gm2, gm3 = gm1 * gm1 % P, gm1 * gm1 * gm1 % P
        p0 = (f_x - 1) * _inv((x - 1) % P) % P
        p1 = (f_x - public_last % P) * _inv((x - gm2) % P) % P
        num = (f_ggx - f_gx * f_gx - f_x * f_x) % P
        den = (pow(x, n, P) - 1) * _inv((x - gm3) * (x - gm2) * (x - gm1) % P) % P
        p2 = num * _inv(den) % P
        cp_sent = val(0, 0) if coset else tuple(cpw)
        if tuple((alpha[j] % P * p0 + alpha[2 + j] % P * p1 + alpha[4 + j] % P * p2) % P for j in (0, 1)) != cp_sent:
            return -2
        if any(len(pth) != L - ce[0] for pth in fp) or (not coset and len(cpp) != L - ce[1]):
            return -3
        for i, idx in enumerate((tp, tp + B, tp + 2 * B)):
            if f_misses(fv[i], idx, fp[i]):
                return -(4 + i)
        if not coset and misses(cpw, tp, cpp, caps[0]):
            return -7
        for j, (r0, steps) in enumerate(grp):
            v = [reduce(val(j, t)) for t in range(1 << steps)]
            xk, om, bk = pow(x, 1 << r0, P), pow(h, N >> steps, P), reduce(betas[j])
            for _ in range(steps):
                cnt = len(v) // 2
                nv = []
                for t in range(cnt):
                    i2x = _inv(2 * xk * pow(om, t, P) % P)
                    hx = mul(bk, tuple((a - b) * i2x % P for a, b in zip(v[t], v[t + cnt])))
                    nv.append(tuple(((a + b) * inv2 + d) % P for a, b, d in zip(v[t], v[t + cnt], hx)))
                v, xk, om, bk = nv, xk * xk % P, om * om % P, mul(bk, bk)
            if j + 1 < G:
                expect = val(j + 1, 0)
            elif not D:
                expect = (coef[0], coef[1])
            else:
                xs, acc = pow(x, 1 << Rp, P), [0, 0]
                for k in reversed(range(1 << D)):
                    acc = [(acc[comp] * xs + coef[(comp << D) + k] % P) % P for comp in (0, 1)]
                expect = tuple(acc)
            if v[0] != expect:
                return -(100 + j)
        for j, (r0, steps) in enumerate(grp):
            s, size = 1 << steps, N >> r0
            plen = lg[1 + r0] - ce[1 + r0]
            if any(len(pth) != plen for pth in lp[j]):
                return -(200 + j)
            if coset:
                if misses(lw[j], tp % (size >> steps), lp[j][0], caps[j]):
                    return -(300 + j)
                continue
            for t in range(s):
                if misses([lw[j][t], lw[j][s + t]], (tp % size + t * (size // s)) % size, lp[j][t], caps[j]):
                    return -(300 + j) if t == 0 else -(400 + j)
    return -8 if rd.p != len(data) else 0
