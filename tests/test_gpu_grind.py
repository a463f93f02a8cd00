"""Proof-of-work grinding on the GPU (zk_grind, zk_ctx_set_grinding, zk_batch_set_grinding, zk_verifier_set_grinding; DESIGN.md
"Grinding"): the device search against the host search and hashlib, every prover against the proofs tests/grind_ref.py builds
without the library, and the GPU verifier against the CPU's check numbers."""
import hashlib
import random
import struct

import numpy as np
import pytest

import grind_ref
import verify_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}


def test_device_search_equals_host_and_hashlib(zk):
    rng = random.Random(24)
    for g in range(1, 25):
        for i in range(4):
            st = bytes(rng.getrandbits(8) for _ in range(32))
            start = (0, 2**32 - (1 << g) // 2 - 1, rng.getrandbits(40), 2**33 - 7)[i]   # the second and last cross a 2^32 carry
            dev = zk.grind(st, g, start)
            assert dev == zk.grind_host(st, g, start, 16), (g, i)
            assert dev >= start and grind_ref.meets(st, g, dev)
            if g <= 16:
                assert dev == grind_ref.smallest_nonce(st, g, start), (g, i)
    # a state whose nonce 0 already meets the bits; and a start that is itself the answer
    st = next(s for s in (hashlib.sha256(k.to_bytes(4, "little")).digest() for k in range(1 << 16)) if grind_ref.word0(s, 0) >> 24 == 0)
    assert zk.grind(st, 8) == 0 == zk.grind_host(st, 8)
    w = zk.grind(st, 8, 1)
    assert zk.grind(st, 8, w) == w and zk.grind(st, 0, 99) == 99


def _trace(n, a1):
    import zkstark_amd
    return zkstark_amd.trace_fibsq(n - 1, 1, a1)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n", [2, 4, 5, 10, 13])
def test_single_prover_equals_the_reference(zk, orc, log_n, hash_kind):
    for log_b in (1, 3):
        for q in (1, 7):
            for g in (1, 8, 16):
                data, state, last, w = grind_ref.grind_proof(orc, log_n, log_b, q, hash_kind, g)
                with zk.Context(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g) as ctx:
                    p = ctx.prove(_trace(1 << log_n, 3141592))
                    info = ctx.last_transcript()
                assert p.data == data and p.state == state, (log_b, q, g)
                assert (info.grind_bits, info.grind_nonce) == (g, w)
                assert p.check(strict=True) == 0


@pytest.mark.parametrize("g", [8, 16])
def test_single_prover_with_early_launch_and_host_levels(zk, orc, g):
    log_n, log_b = 10, 3
    data, state, _, _ = grind_ref.grind_proof(orc, log_n, log_b, 2, 0, g)
    for early in (False, True):
        for levels in ((0, 0), (8, 9)):
            with zk.Context(log_n, log_b, queries=2, host_levels=levels, grind_bits=g) as ctx:
                ctx.set_early_launch(early)
                p = ctx.prove(_trace(1 << log_n, 3141592))
            assert (p.data, p.state) == (data, state), (early, levels)


def test_default_is_unchanged(zk, orc):
    for log_n, log_b in ((5, 2), (10, 3)):
        r = orc.prove(log_n, log_b, want_vectors=False)
        with zk.Context(log_n, log_b, grind_bits=0) as ctx:
            p = ctx.prove(_trace(1 << log_n, 3141592))
            assert ctx.last_transcript().grind_bits == 0
        assert (p.data, p.state) == (r.proof, r.state)


def test_prove_channel_on_a_prefixed_channel(zk):
    log_n, log_b, g = 10, 3, 12
    ch = zk.Channel()
    ch.commit(b"a transcript prefix of the caller")
    s0 = ch.state
    n0 = len(ch.data)
    with zk.Context(log_n, log_b, grind_bits=g) as ctx:
        ctx.trace_upload(_trace(1 << log_n, 3141592))
        p = ctx.prove_channel(ch)
        w = ctx.last_transcript().grind_nonce
    body = p.data[n0:]
    s = grind_ref.replay_prefix(body, log_n, s0)
    off = grind_ref.prefix_len(log_n)
    assert struct.unpack("<Q", body[off:off + 8])[0] == w == zk.grind_host(s, g)
    assert zk.Proof(p.state, body, log_n, log_b, p.public_last, grind_bits=g).check() == 0
    # the same trace on a fresh channel: the prefix changed the state the nonce was ground on
    with zk.Context(log_n, log_b, grind_bits=g) as ctx:
        fresh = ctx.prove(_trace(1 << log_n, 3141592))
    assert fresh.check(strict=True) == 0 and fresh.data != body


@pytest.mark.parametrize("q", [1, 16])
def test_batch_prover_equals_the_single_prover(zk, q):
    log_n, log_b = 6, 2
    for g in (8, 16):
        for log_batch in range(5):
            a1s = [3141592 + 7 * p for p in range(1 << log_batch)]
            with zk.BatchContext(log_n, log_b, log_batch, queries=q, grind_bits=g) as bc:
                bc.gen_fibsq([1] * len(a1s), a1s)
                got = bc.prove()
            with zk.Context(log_n, log_b, queries=q, grind_bits=g) as ctx:
                for p, a1 in zip(got, a1s):
                    want = ctx.prove(_trace(1 << log_n, a1))
                    assert (p.data, p.state) == (want.data, want.state), (g, log_batch, a1)
                    assert p.check(strict=True) == 0


def _relaid_corpus(orc, log_n, log_b, q, h, g):
    """The tamper corpus of tests/verify_corpus.py on grinding proofs: each proof without its nonce goes through
    verify_corpus.variants (the g = 0 layout), then every variant gets its proof's nonce back; plus the nonce tampers."""
    off = grind_ref.prefix_len(log_n)
    proofs = [grind_ref.grind_proof(orc, log_n, log_b, q, h, g, a1=a1) for a1 in verify_corpus.SEEDS]
    stripped = [(d[:off] + d[off + 8:], s, last) for d, s, last, _ in proofs]
    items = []
    for it in verify_corpus.variants(stripped, log_n, log_b, q):
        k = int(it.label[1]) if it.label.startswith("p") else None
        nonce = proofs[k][0][off:off + 8] if k is not None else it.data[:8]
        items.append(verify_corpus.Item(it.label, it.data[:off] + nonce + it.data[off:], it.state, it.public_last))
    for k, (d, s, last, w) in enumerate(proofs):
        st = grind_ref.replay_prefix(d, log_n)
        bad = next(v for v in range(w + 1, w + 10**6) if not grind_ref.meets(st, g, v))
        nxt = grind_ref.smallest_nonce(st, g, w + 1)
        for label, v in (("nonce.fails", bad), ("nonce.next", nxt)):
            items.append(verify_corpus.Item(f"p{k}.{label}", d[:off] + struct.pack("<Q", v) + d[off + 8:], s, last))
    return items


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g", [(5, 2, 1, 8), (5, 2, 3, 16), (10, 3, 1, 4)])
def test_gpu_verifier_equals_the_cpu(zk, orc, log_n, log_b, q, g, hash_kind):
    items = _relaid_corpus(orc, log_n, log_b, q, hash_kind, g)
    data = np.stack([np.frombuffer(it.data, dtype=np.uint8) for it in items])
    seen = set()
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g) as v:
        for strict in (True, False):
            want = np.array([zk.Proof(it.state, it.data, log_n, log_b, it.public_last, HASH_NAMES[hash_kind], q, g).check(strict)
                             for it in items], dtype=np.int32)
            states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
            got = v.verify_raw(data, [it.public_last for it in items], states)
            bad = [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
            assert not bad, (strict, bad)
            seen |= set(want.tolist())
            labels = {it.label: int(c) for it, c in zip(items, want)}
            assert labels["p0.valid"] == 0
            assert labels["p0.nonce.fails"] == (-1998 if strict else 0)
            assert labels["p0.nonce.next"] == (-(1000 + 3 + log_n + 1) if strict else 0)
    assert -1998 in seen and -1999 in seen and -2 in seen and len(seen) > 10


def test_setters_refuse_more_than_32_bits(zk):
    from zkstark_amd import _lib
    for make in (lambda g: zk.Context(5, 2, grind_bits=g), lambda g: zk.BatchContext(5, 2, 2, grind_bits=g),
                 lambda g: zk.Verifier(5, 2, grind_bits=g)):
        with pytest.raises(zk.ZkError) as e:
            make(33)
        assert e.value.code == -1
        make(32).close()
    with pytest.raises(zk.ZkError):
        zk.grind(bytes(32), 33)
    assert _lib.load().zk_proof_data_len_grind(5, 2, 1, 32) == _lib.load().zk_proof_data_len_queries(5, 2, 1) + 8


def test_benchmark_domain_2e24(zk):
    """One 2^24-point proof (log_n 21) with g = 20: strict CPU verification, and the nonce is the host search's."""
    log_n, log_b, g = 21, 3, 20
    with zk.Context(log_n, log_b, grind_bits=g) as ctx:
        p = ctx.prove(zk.trace_fibsq((1 << log_n) - 1))
        w = ctx.last_transcript().grind_nonce
    off = grind_ref.prefix_len(log_n)
    assert struct.unpack("<Q", p.data[off:off + 8])[0] == w
    assert w == zk.grind_host(grind_ref.replay_prefix(p.data, log_n), g)
    assert p.check(strict=True) == 0
    p.verify(strict=True)


def test_transcript_info_layouts(zk):
    """zk_transcript_info grew at its end: a caller with the version-6 layout (1244 bytes) gets its fields and nothing past
    them; the full layout gets grind_bits and grind_nonce; a size between the two is refused before anything is written."""
    import ctypes as C
    from zkstark_amd import _lib
    lib = _lib.load()

    class V6(C.Structure):
        _fields_ = [f for f in _lib.TranscriptInfo._fields_ if not f[0].startswith("grind_")] + [("after", C.c_uint8 * 16)]

    with zk.Context(10, 3, grind_bits=16) as ctx:
        p = ctx.prove(zk.trace_fibsq(1023))
        full = ctx.last_transcript()
        off = grind_ref.prefix_len(10)
        assert full.grind_bits == 16 and full.grind_nonce == struct.unpack("<Q", p.data[off:off + 8])[0]
        old = V6()
        old.struct_size = 1244
        C.memset(C.byref(old, 1244), 0xAB, 16)
        assert lib.zk_last_transcript(ctx._h, C.cast(C.pointer(old), C.POINTER(_lib.TranscriptInfo))) == 0
        assert old.public_last == full.public_last and old.free_term == full.free_term and bytes(old.after) == b"\xab" * 16
        for n in (1245, 1248, 1252, 1255):
            old.struct_size = n
            old.free_term = 4242
            assert lib.zk_last_transcript(ctx._h, C.cast(C.pointer(old), C.POINTER(_lib.TranscriptInfo))) == -1 and old.free_term == 4242, n
