"""Tamper corpus for the verifier tests (tests/test_verify_check.py, tests/test_gpu_verify_batch.py).

For each valid proof it makes one variant per field of the wire format (transcript.hpp: proof_data_len / verify_proof):
the f root, each alpha, the cp root, each beta and layer root, the free term, each query raw, and per query each value, one
node of each path and each count field.  Every variant comes in three kinds: one bit flipped; the value plus P (a raw value
>= P with the same residue; for a digest its first word, for a count the u64); and a swap with the same field of another
proof of the batch.  Then a wrong public_last (public_last + 1, + P, with the top bit flipped), a wrong state, an all-zero
proof and random bytes (the random bytes break the path counts: the malformed-layout path of the batched verifier).
"""
import struct

import numpy as np

P = 3221225473
SEEDS = (3141592, 3141593)          # a1 of the two proofs of every batch (a0 = 1)


class Item:
    """One proof to check: its bytes, Proof.state and public_last, and what was done to it."""

    def __init__(self, label, data, state, public_last):
        self.label, self.data, self.state, self.public_last = label, bytes(data), bytes(state), public_last & 0xFFFFFFFF


def proof_len(log_n, log_b, q):
    L, R = log_n + log_b, log_n
    per_query = 4 + 4 * (4 + 8 + 32 * L) + sum(8 + 2 * (8 + 32 * (L - i)) for i in range(R))
    return 32 + 12 + 32 + R * 36 + 4 + q * per_query


def fields(log_n, log_b, q):
    """(name, byte offset, size, kind) of every field the corpus touches; kind is "value" (u32), "digest" (32 bytes), "count" (u64)."""
    L, R = log_n + log_b, log_n
    out = [("f_root", 0, 32, "digest")]
    out += [(f"alpha{i}", 32 + 4 * i, 4, "value") for i in range(3)]
    out.append(("cp_root", 44, 32, "digest"))
    for i in range(R):
        out.append((f"beta{i}", 76 + 36 * i, 4, "value"))
        out.append((f"layer_root{i}", 80 + 36 * i, 32, "digest"))
    out.append(("free_term", 76 + 36 * R, 4, "value"))
    qraw = 80 + 36 * R
    out += [(f"query_raw{k}", qraw + 4 * k, 4, "value") for k in range(q)]
    per_q = 4 * (12 + 32 * L) + sum(24 + 64 * (L - i) for i in range(R))
    for k in range(q):
        base = qraw + 4 * q + k * per_q
        for j in range(4):                                   # f(x), f(gx), f(g^2 x), cp(x)
            b = base + j * (12 + 32 * L)
            node = (k + j) % L
            out += [(f"q{k}.f{j}.value", b, 4, "value"), (f"q{k}.f{j}.count", b + 4, 8, "count"),
                    (f"q{k}.f{j}.node{node}", b + 12 + 32 * node, 32, "digest")]
        lb = base + 4 * (12 + 32 * L)
        for i in range(R):
            plen = L - i
            node = (k + i) % plen
            out += [(f"q{k}.layer{i}.x", lb, 4, "value"), (f"q{k}.layer{i}.nx", lb + 4, 4, "value"),
                    (f"q{k}.layer{i}.x_count", lb + 8, 8, "count"), (f"q{k}.layer{i}.x_node{node}", lb + 16 + 32 * node, 32, "digest"),
                    (f"q{k}.layer{i}.nx_count", lb + 16 + 32 * plen, 8, "count"),
                    (f"q{k}.layer{i}.nx_node{node}", lb + 24 + 32 * plen + 32 * node, 32, "digest")]
            lb += 24 + 64 * plen
    assert lb == proof_len(log_n, log_b, q)
    return out


def _plus_p(b, kind):
    """The field with P added (a raw word >= P that has the same residue), or None where that does not fit the field."""
    if kind == "count":
        return struct.pack("<Q", (struct.unpack("<Q", b)[0] + P) & (2**64 - 1))
    if kind == "value":
        v = struct.unpack("<I", b)[0]
        return struct.pack("<I", v + P) if v + P < 2**32 else None
    w = struct.unpack(">I", b[:4])[0]                        # digest: its first (big-endian) state word
    return struct.pack(">I", w + P) + b[4:] if w + P < 2**32 else None


def variants(proofs, log_n, log_b, q, rng_seed=0):
    """proofs: [(data, state, public_last)] of one size (at least two).  Returns the valid proofs and every variant as Items."""
    out = []
    for i, (data, state, last) in enumerate(proofs):
        other = proofs[(i + 1) % len(proofs)][0]
        out.append(Item(f"p{i}.valid", data, state, last))
        for name, off, size, kind in fields(log_n, log_b, q):
            field = data[off:off + size]
            bit = (off * 7 + i) % (8 * size)
            flipped = bytearray(field)
            flipped[bit // 8] ^= 1 << (bit % 8)
            kinds = [("flip", bytes(flipped)), ("plusP", _plus_p(field, kind)), ("swap", other[off:off + size])]
            for how, new in kinds:
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


def oracle_proofs(orc, log_n, log_b, q, hash_kind):
    """Two valid proofs of one size from the CPU oracle: [(data, state, public_last)]."""
    orc.set_queries(q)
    orc.set_hash(hash_kind)
    try:
        out = []
        for a1 in SEEDS:
            r = orc.prove(log_n, log_b, 1, a1, want_vectors=False)
            assert r.rc == 0
            out.append((r.proof, r.state, r.public_last))
        return out
    finally:
        orc.set_queries(1)
        orc.set_hash(0)


def corpus(orc, log_n, log_b, q, hash_kind):
    return variants(oracle_proofs(orc, log_n, log_b, q, hash_kind), log_n, log_b, q)
