"""Coset leaves without a GPU: the proof length, the CPU verifier zk_verify_coset against the plain-Python verifier
of tests/coset_ref.py -- accepted proofs and, for tampered ones, the same check number -- and zk_compute_root_from_coset against the
Python tree."""
import ctypes as C

import numpy as np
import pytest

import coset_ref
import fold_ref

P = coset_ref.P


def _check(lib, data, state, log_n, log_b, last, h, q, g, K, fn="zk_verify_coset"):
    out = C.c_int32(12345)
    rc = getattr(lib, fn)(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value)
    return out.value


def test_proof_length(zk):
    lib = zk.load()
    for log_n in (2, 4, 5, 6, 7, 8, 9, 10, 11, 12):
        for log_b in (1, 2, 3):
            for q in (1, 3):
                for g in (0, 8):
                    for K in (1, 2, 3):
                        assert lib.zk_proof_data_len_coset(log_n, log_b, q, g, K) == coset_ref.proof_len(log_n, log_b, q, g, K)
    assert lib.zk_proof_data_len_coset(10, 3, 1, 0, 0) == 0 and lib.zk_proof_data_len_coset(10, 3, 1, 0, 4) == 0
    # the sizes the header and DESIGN.md quote, next to those of one-value leaves
    assert [lib.zk_proof_data_len_coset(21, 3, 1, 0, K) for K in (1, 2, 3)] == [12252, 7332, 5644]
    assert [lib.zk_proof_data_len_coset(21, 3, 32, 0, K) for K in (1, 2, 3)] == [366148, 219868, 170316]
    assert [lib.zk_proof_data_len_coset(10, 3, 1, 0, K) for K in (1, 2, 3)] == [4288, 2788, 2416]
    assert [coset_ref.proof_len(21, 3, 1, 0, K) for K in (1, 2, 3)] == [12252, 7332, 5644]
    assert [coset_ref.proof_len(21, 3, 32, 0, K) for K in (1, 2, 3)] == [366148, 219868, 170316]
    assert [coset_ref.proof_len(10, 3, 1, 0, K) for K in (1, 2, 3)] == [4288, 2788, 2416]


SIZES = [(2, 1), (4, 1), (5, 2), (6, 3), (10, 3)]           # short last group: 4 / K=3, 5 / K=2, 5 / K=3, 10 / K=3; two-leaf trees at log_b 1


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_cpu_verifier_accepts_reference_proofs(zk, orc, K, hash_kind):
    lib = zk.load()
    for log_n, log_b in SIZES:
        for q in (1, 3):
            for g in (0, 8):
                ref = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, g)
                assert len(ref.data) == lib.zk_proof_data_len_coset(log_n, log_b, q, g, K)
                args = (log_n, log_b, ref.public_last, hash_kind, q, g, K)
                assert coset_ref.verify(orc, ref.data, ref.state, *args) == 0, args
                assert coset_ref.verify(orc, ref.data, None, *args) == 0, args
                assert _check(lib, ref.data, ref.state, *args) == 0, args
                assert _check(lib, ref.data, None, *args) == 0, args


def _tampered(ref, log_n, log_b, q, g, K):
    """(name, bytes) of every tampering of a coset proof: one flipped byte per region, a swapped slot pair inside every leaf,
    one byte less, one byte more."""
    data = ref.data
    for name, off, n in coset_ref.regions(log_n, log_b, q, g, K):
        pos = off + (n // 2 if n > 8 else 0)                # a u64 count: its low byte; a digest / path: a byte in the middle
        bad = bytearray(data)
        bad[pos] ^= 0x01 if name.endswith(".count") else 0x40
        yield name, bytes(bad)
        if name.endswith(".slot0"):                         # slots 0 and 1 of this leaf exchanged
            bad = bytearray(data)
            bad[off:off + 4], bad[off + 4:off + 8] = data[off + 4:off + 8], data[off:off + 4]
            if bytes(bad) != data:
                yield name + "<->slot1", bytes(bad)
    name, off, n = [r for r in coset_ref.regions(log_n, log_b, q, g, K) if r[0].endswith(".count")][-1]
    bad = bytearray(data)                                   # the last path announces one digest less: its length check, not the parser
    bad[off] -= 1
    yield "last count - 1", bytes(bad)
    yield "truncated", data[:-1]
    yield "appended", data + b"\0"


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,K,q,g", [(5, 2, 2, 2, 0), (6, 3, 3, 1, 8)])
def test_tampered_proofs_get_the_same_check_number(zk, orc, log_n, log_b, K, q, g, hash_kind):
    lib = zk.load()
    ref = coset_ref.coset_proof(orc, log_n, log_b, q, hash_kind, K, g)
    args = (log_n, log_b, ref.public_last, hash_kind, q, g, K)
    seen = set()
    for name, bad in _tampered(ref, log_n, log_b, q, g, K):
        for state in (ref.state, None):
            want = coset_ref.verify(orc, bad, state, *args)
            got = _check(lib, bad, state, *args)
            assert got == want, (name, state is not None, got, want)
            seen.add(got)
            if state is not None or not (name.startswith(("alpha", "beta", "raw", "nonce")) or name == "root%d" % len(fold_ref.groups(log_n, K))):
                # lax mode reads challenges from the proof (as the reference does) and never opens the last tree
                assert got != 0 or name in ("nonce",), (name, state is not None)
    # the checks the format has all occur, those it does not have never do
    G = len(fold_ref.groups(log_n, K))
    assert {-1, -2, -4, -5, -6, -8, -100, -(200 + G - 1), -300} <= seen, sorted(seen)
    assert not any(c == -7 or -500 < c <= -400 for c in seen), sorted(seen)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_formats_reject_each_other_by_length(zk, orc, K):
    lib = zk.load()
    for log_n, log_b in ((5, 2), (6, 3)):
        coset = coset_ref.coset_proof(orc, log_n, log_b, 1, 0, K)
        plain = fold_ref.fold_proof(orc, log_n, log_b, 1, 0, K)
        assert coset.public_last == plain.public_last
        for state in (True, False):
            assert _check(lib, coset.data, coset.state if state else None, log_n, log_b, coset.public_last, 0, 1, 0, K, "zk_verify_fold") == -1
            assert _check(lib, plain.data, plain.state if state else None, log_n, log_b, plain.public_last, 0, 1, 0, K) == -1


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
def test_compute_root_from_coset(zk, orc, hash_kind):
    lib = zk.load()
    rng = np.random.default_rng(7)
    layer = rng.integers(0, P, 64, dtype=np.uint64).astype(np.uint32)
    layer[:3] = (0, P - 1, 1)
    orc.set_hash(hash_kind)
    try:
        for steps in (0, 1, 2, 3):
            s, m = 1 << steps, 64 >> steps
            nodes = coset_ref.tree(orc, layer, steps, hash_kind)
            if steps == 0:
                assert np.array_equal(nodes, orc.merkle_build(layer))   # s = 1 is the one-value leaf
            for leaf in range(m):
                slots = np.array([layer[leaf + u * m] for u in range(s)], dtype=np.uint32)
                pth = coset_ref.path(nodes, leaf)
                out = C.create_string_buffer(32)
                assert lib.zk_compute_root_from_coset(slots.ctypes.data_as(C.c_void_p), s, leaf, b"".join(pth), len(pth), out, hash_kind) == 0
                assert out.raw == bytes(nodes[0]), (steps, leaf)
                assert zk.compute_root_from_coset(slots, leaf, pth, "field" if hash_kind else "sha256") == bytes(nodes[0])
                assert coset_ref.root_from_leaf(orc, list(slots), leaf, pth, hash_kind) == bytes(nodes[0])
                if steps == 0:
                    ex = C.create_string_buffer(32)
                    assert lib.zk_compute_root_from_path_ex(int(slots[0]), leaf, b"".join(pth), len(pth), ex, hash_kind) == 0 and ex.raw == out.raw
    finally:
        orc.set_hash(0)
    bad = C.create_string_buffer(32)
    assert lib.zk_compute_root_from_coset(layer.ctypes.data_as(C.c_void_p), 3, 0, b"", 0, bad, 0) != 0   # s must be 1, 2, 4 or 8
