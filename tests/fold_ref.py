"""Proofs with a FRI folding factor 2^K built without the library, and a plain-Python verifier of the same format
(tests/test_fold_arity.py, tests/test_gpu_fold_arity.py; DESIGN.md "Folding factor").

The CPU oracle gives the trace, f and (on a fresh channel) cp; everything after that is assembled here from the oracle's
primitives: the channel is replayed with hashlib, a group of `steps` rounds draws one challenge beta and is folded by `steps`
calls of orc.fri_fold_eval with beta, beta^2, beta^4, only the group outputs get a tree (orc.merkle_build after orc.set_hash),
then the free term, the optional nonce (grind_ref.smallest_nonce), the query raws and the openings: per group the s = 2^steps
values of its input layer at (x % len + t len / s) % len, then their s paths.  With K = 1 the bytes are oracle.prove's."""
import functools
import hashlib
import struct

import numpy as np

import grind_ref

P = 3221225473
GEN_W = 5


def groups(log_n, K):
    """[(r0, steps)] of the groups the log_n rounds are taken in."""
    return [(r0, min(K, log_n - r0)) for r0 in range(0, log_n, K)]


def proof_len(log_n, log_b, q, bits, K):
    L = log_n + log_b
    per_query = 4 + 4 * (12 + 32 * L) + sum((1 << s) * (12 + 32 * (L - r0)) for r0, s in groups(log_n, K))
    return 32 + 12 + 32 + 36 * len(groups(log_n, K)) + 4 + (8 if bits else 0) + q * per_query


class _Channel:
    """channel.rs:6-37 on hashlib."""

    def __init__(self, prefix=b""):
        self.state, self.data = bytes(32), bytearray()
        if prefix:
            self.commit(prefix)

    def commit(self, b):
        self.state = hashlib.sha256(self.state + bytes(b)).digest()
        self.data += b

    def get_u32(self):
        v = struct.unpack(">I", self.state[:4])[0]
        self.commit(struct.pack("<I", v))
        return v


class Folded:
    """What a folded proof commits to: layers[id] / trees[id] for the committed ids (0 = f, 1 = cp, 1 + r0 + steps per group),
    betas[r0], roots[id], and the channel after the free term."""


def fold_layer(orc, layer, log_n, log_b, r0, steps, beta_raw):
    """`steps` reference folds of rounds r0, r0 + 1, ... with the challenges beta, beta^2, beta^4 (beta reduced mod P first)."""
    b = beta_raw % P
    for t in range(steps):
        layer = orc.fri_fold_eval(layer, log_n, log_b, r0 + t, b)
        b = b * b % P
    return layer


@functools.lru_cache(maxsize=4)
def committed(orc, log_n, log_b, hash_kind, K, a1=3141592, prefix=b""):
    """The transcript up to and including the free term, with every committed layer and tree."""
    r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
    assert r.rc == 0
    c = Folded()
    c.public_last, c.layers, c.trees, c.roots, c.betas = r.public_last, {}, {}, {}, {}
    ch = _Channel(prefix)
    orc.set_hash(hash_kind)
    try:
        def commit_layer(i, vals):
            c.layers[i] = np.array(vals, dtype=np.uint32)
            c.trees[i] = orc.merkle_build(c.layers[i])
            c.roots[i] = bytes(c.trees[i][0])
            ch.commit(c.roots[i])

        commit_layer(0, r.f_eval)
        c.alphas = [ch.get_u32() for _ in range(3)]
        commit_layer(1, orc.compose(r.f_eval, log_n, log_b, c.alphas, r.public_last))
        if not prefix and hash_kind == 0:
            assert bytes(ch.data) == r.proof[:76] and np.array_equal(c.layers[1], r.cp_layers[0])
        for r0, steps in groups(log_n, K):
            beta = c.betas[r0] = ch.get_u32()
            commit_layer(1 + r0 + steps, fold_layer(orc, c.layers[1 + r0], log_n, log_b, r0, steps, beta))
    finally:
        orc.set_hash(0)
    last = c.layers[1 + log_n]
    assert len(last) == 1 << log_b and len(set(int(v) for v in last)) == 1
    c.free_term = int(last[0])
    ch.commit(struct.pack("<I", c.free_term))
    c.prefix_state, c.prefix_data = ch.state, bytes(ch.data)
    return c


def _path(orc, nodes, leaf):
    return b"".join(bytes(row) for row in orc.merkle_trace(nodes, leaf))


class RefProof:
    pass


def fold_proof(orc, log_n, log_b, q, hash_kind, K, bits=0, a1=3141592, prefix=b""):
    """The proof of fibsq(1, a1) folded by 2^K: .data (Channel.data, the prefix included), .state, .public_last, .nonce, .c (Folded)."""
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
        for lid, idx in ((0, x), (0, x + B), (0, x + 2 * B), (1, x)):
            ch.commit(struct.pack("<IQ", int(c.layers[lid][idx]), L) + _path(orc, c.trees[lid], idx))
        for r0, steps in groups(log_n, K):
            s, size = 1 << steps, N >> r0
            idx = [(x % size + t * (size // s)) % size for t in range(s)]
            layer, tree = c.layers[1 + r0], c.trees[1 + r0]
            ch.commit(b"".join(struct.pack("<I", int(layer[i])) for i in idx)
                      + b"".join(struct.pack("<Q", L - r0) + _path(orc, tree, i) for i in idx))
    out.data, out.state, out.raws = bytes(ch.data), ch.state, raws
    return out


# ---- the verifier (proof.rs:15-149 widened), in plain Python -------------------------------------------------------------------
class _Short(Exception):
    pass


class _Reader:
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, n):
        if len(self.d) - self.p < n:
            self.p = len(self.d)
            raise _Short()
        b = self.d[self.p:self.p + n]
        self.p += n
        return b

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def path(self):
        cnt = struct.unpack("<Q", self.take(8))[0]
        if cnt > 64:
            raise _Short()
        return [self.take(32) for _ in range(cnt)]


def _inv(a):
    return pow(a, P - 2, P)


def _root_from_path(orc, element, index, path):
    return orc.compute_root_from_path(element, index, np.frombuffer(b"".join(path), dtype=np.uint8).reshape(len(path), 32))


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
        for _ in range(4):
            ch.commit(rd.take(12 + 32 * L))
        for r0, steps in groups(log_n, K):
            ch.commit(rd.take((1 << steps) * (12 + 32 * (L - r0))))
    return 0 if ch.state == bytes(state) else -1999


def verify(orc, data, state, log_n, log_b, public_last, hash_kind, q, bits, K):
    """The check number of the folded-proof verifier: strict (the replay first) when state is not None."""
    if state is not None:
        rc = replay(data, state, log_n, log_b, q, bits, K)
        if rc:
            return rc
    orc.set_hash(hash_kind)
    try:
        return _verify(orc, data, log_n, log_b, public_last, q, bits, K)
    finally:
        orc.set_hash(0)


def _verify(orc, data, log_n, log_b, public_last, q, bits, K):
    n, L = 1 << log_n, log_n + log_b
    N, B = 1 << L, 1 << log_b
    grp = groups(log_n, K)
    G = len(grp)
    rd = _Reader(data)
    short = False
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
        return -1                                           # q >= 1: the first query finds the header short
    g, h = pow(GEN_W, (P - 1) >> log_n, P), pow(GEN_W, (P - 1) >> L, P)
    inv2 = _inv(2)
    for raw in raws:
        try:
            fv, fp = [], []
            for _ in range(4):
                fv.append(rd.u32())
                fp.append(rd.path())
            lv, lp = [], []
            for r0, steps in grp:
                lv.append([rd.u32() for _ in range(1 << steps)])
                lp.append([rd.path() for _ in range(1 << steps)])
        except _Short:
            return -1
        tp = raw % (N - 2 * B)
        x = GEN_W * pow(h, tp, P) % P
        f_x, f_gx, f_ggx = fv[0] % P, fv[1] % P, fv[2] % P
        gm1 = _inv(g)
        gm2, gm3 = gm1 * gm1 % P, gm1 * gm1 * gm1 % P
        p0 = (f_x - 1) * _inv((x - 1) % P) % P
        p1 = (f_x - public_last % P) * _inv((x - gm2) % P) % P
        num = (f_ggx - f_gx * f_gx - f_x * f_x) % P
        den = (pow(x, n, P) - 1) * _inv((x - gm3) * (x - gm2) * (x - gm1) % P) % P
        p2 = num * _inv(den) % P
        if (alpha[0] % P * p0 + alpha[1] % P * p1 + alpha[2] % P * p2) % P != fv[3]:
            return -2
        if any(len(p) != L for p in fp):
            return -3
        for i, (idx, root) in enumerate(((tp, f_root), (tp + B, f_root), (tp + 2 * B, f_root), (tp, roots[0]))):
            if _root_from_path(orc, fv[i], idx, fp[i]) != root:
                return -(4 + i)
        for j, (r0, steps) in enumerate(grp):               # the s opened values folded pairwise: t with t + s/2, then again
            v = [a % P for a in lv[j]]
            xk, om, bk = pow(x, 1 << r0, P), pow(h, N >> steps, P), betas[j] % P
            for _ in range(steps):
                cnt = len(v) // 2
                v = [((v[t] + v[t + cnt]) * inv2 + bk * (v[t] - v[t + cnt]) * _inv(2 * xk * pow(om, t, P) % P)) % P for t in range(cnt)]
                xk, om, bk = xk * xk % P, om * om % P, bk * bk % P
            if v[0] != (lv[j + 1][0] if j + 1 < G else free_term):
                return -(100 + j)
        for j, (r0, steps) in enumerate(grp):
            s, size = 1 << steps, N >> r0
            if any(len(p) != L - r0 for p in lp[j]):
                return -(200 + j)
            for t in range(s):
                if _root_from_path(orc, lv[j][t], (tp % size + t * (size // s)) % size, lp[j][t]) != roots[j]:
                    return -(300 + j) if t == 0 else -(400 + j)
    return -8 if rd.p != len(data) else 0
