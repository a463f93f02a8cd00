"""Grinding proofs built without the library (tests/test_grind.py, tests/test_gpu_grind.py; DESIGN.md "Grinding").

The CPU oracle's proof up to and including the free term is unchanged by grinding.  From there: the channel is replayed with
hashlib, the smallest nonce found by a hashlib scan (keep g <= 16 here), committed, the q query raws drawn, and the openings
assembled from the layers the same oracle call returns (res.f_eval, res.cp_layers), their trees (orc.merkle_build, after
orc.set_hash) and their paths (orc.merkle_trace)."""
import functools
import hashlib
import struct


def word0(state, nonce):
    """Digest word 0 (big-endian) of SHA-256(state || le64(nonce))."""
    return struct.unpack(">I", hashlib.sha256(bytes(state) + struct.pack("<Q", nonce)).digest()[:4])[0]


def meets(state, bits, nonce):
    return bits == 0 or word0(state, nonce) >> (32 - bits) == 0


def smallest_nonce(state, bits, start=0):
    w = start
    while not meets(state, bits, w):
        w += 1
    return w


def prefix_len(log_n):
    return 32 + 12 + 32 + 36 * log_n + 4


def replay_prefix(data, log_n, state=bytes(32)):
    """Channel state after the f root, the alphas, the cp root, the R (beta, layer root) pairs and the free term, from `state`."""
    st = bytes(state)
    pos = 0
    for n in [32, 4, 4, 4, 32] + [4, 32] * log_n + [4]:
        st = hashlib.sha256(st + data[pos:pos + n]).digest()
        pos += n
    return st


@functools.lru_cache(maxsize=None)
def _oracle(orc, log_n, log_b, hash_kind, a1):
    orc.set_hash(hash_kind)
    try:
        r = orc.prove(log_n, log_b, 1, a1, want_vectors=True)
        assert r.rc == 0
        trees = [orc.merkle_build(r.f_eval)] + [orc.merkle_build(layer) for layer in r.cp_layers[:log_n]]
    finally:
        orc.set_hash(0)
    return r, trees


def _path(orc, nodes, leaf):
    """merkle.rs:54-71 as the bytes of the path (sibling of the leaf first)."""
    return b"".join(bytes(row) for row in orc.merkle_trace(nodes, leaf))


def grind_proof(orc, log_n, log_b, q, hash_kind, bits, a1=3141592, nonce=None):
    """(data, state, public_last, nonce) of the grinding proof of fibsq(1, a1); nonce=None: the smallest one, else the given nonce
    (which must meet the bits for the proof to be the prover's)."""
    r, trees = _oracle(orc, log_n, log_b, hash_kind, a1)
    L, R = log_n + log_b, log_n
    N, B = 1 << L, 1 << log_b
    data = bytearray(r.proof[:prefix_len(log_n)])
    st = replay_prefix(data, log_n)
    if bits:
        w = smallest_nonce(st, bits) if nonce is None else nonce
        enc = struct.pack("<Q", w)
        st = hashlib.sha256(st + enc).digest()
        data += enc
    else:
        w = None
    raws = []
    for _ in range(q):
        raw = struct.unpack(">I", st[:4])[0]
        enc = struct.pack("<I", raw)
        st = hashlib.sha256(st + enc).digest()
        data += enc
        raws.append(raw)

    def commit(b):
        nonlocal st
        st = hashlib.sha256(st + b).digest()
        data.extend(b)

    for raw in raws:
        x = raw % (N - 2 * B)
        for layer, tree, idx in ((r.f_eval, trees[0], x), (r.f_eval, trees[0], x + B), (r.f_eval, trees[0], x + 2 * B),
                                 (r.cp_layers[0], trees[1], x)):
            commit(struct.pack("<IQ", int(layer[idx]), L) + _path(orc, tree, idx))
        for i in range(R):
            size = N >> i
            xi, nx = x % size, (x % size + size // 2) % size
            layer, tree = r.cp_layers[i], trees[1 + i]
            pl = L - i
            commit(struct.pack("<II", int(layer[xi]), int(layer[nx])) + struct.pack("<Q", pl) + _path(orc, tree, xi)
                   + struct.pack("<Q", pl) + _path(orc, tree, nx))
    return bytes(data), st, r.public_last, w
