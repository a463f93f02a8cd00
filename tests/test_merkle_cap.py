"""Merkle caps without a GPU (zk_verify_cap, zk_proof_data_len_cap): the proof length against tests/cap_ref.py over the
whole admissible grid, the CPU verifier against the plain-Python one -- accepted proofs and, for tampered ones, the same check
number -- cap 0 being zk_verify_stop / zk_proof_data_len_stop, proofs of another cap rejected by length, and the setters' refusals."""
import ctypes as C
import re

import pytest

import cap_ref
import stop_ref

CAPS = range(0, 9)


def _check(lib, data, state, log_n, log_b, last, h, q, g, K, coset, D, c):
    out = C.c_int32(12345)
    rc = lib.zk_verify_cap(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, int(coset), D, c, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value)
    return out.value


def test_proof_length_grid(zk):
    lib = zk.load()
    n = 0
    for log_n in range(2, 13):
        for log_b in range(1, 6):
            for q in (1, 3, 64):
                for K in (1, 2, 3):
                    for coset in (0, 1):
                        for D in range(0, 10):
                            ok = stop_ref.admissible(log_n, log_b, D)
                            for c in CAPS:
                                got = lib.zk_proof_data_len_cap(log_n, log_b, q, 0, K, coset, D, c)
                                if not ok:
                                    assert got == 0, (log_n, log_b, q, K, coset, D, c)
                                    continue
                                assert got == cap_ref.proof_len(log_n, log_b, q, 0, K, coset, D, c), (log_n, log_b, q, K, coset, D, c)
                                n += c > 0
                            if ok:
                                assert lib.zk_proof_data_len_cap(log_n, log_b, q, 0, K, coset, D, 0) == lib.zk_proof_data_len_stop(log_n, log_b, q, 0, K, coset, D)
    assert n > 50000
    assert lib.zk_proof_data_len_cap(10, 3, 1, 0, 1, 0, 0, 9) == 0 and lib.zk_proof_data_len_cap(10, 3, 1, 0, 4, 0, 0, 2) == 0
    assert lib.zk_proof_data_len_cap(10, 3, 3, 5, 2, 1, 2, 4) == cap_ref.proof_len(10, 3, 3, 5, 2, True, 2, 4)   # grinding: 8 bytes, as ever
    # the sizes of DESIGN.md 7f, domain 2^24
    assert [lib.zk_proof_data_len_cap(21, 3, 32, 0, 1, 0, 0, c) for c in (0, 2, 4, 5, 6, 8)] == [719044, 627044, 543076, 510308, 488804, 519524]
    assert [lib.zk_proof_data_len_cap(21, 3, 32, 0, 3, 1, 6, c) for c in (0, 2, 4, 5, 6, 8)] == [158688, 142880, 128800, 123680, 121632, 142112]
    assert [lib.zk_proof_data_len_cap(21, 3, 1, 0, 1, 0, 0, c) for c in (0, 2, 4)] == [23280, 22544, 27856]


def test_reference_cap0_is_the_plain_reference(orc):
    for log_n, log_b, q, h, K, coset, D in ((4, 1, 1, 0, 1, False, 0), (6, 3, 3, 1, 2, True, 2), (6, 3, 2, 0, 3, False, 0), (5, 2, 2, 0, 1, True, 1)):
        assert cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, 0, 5).data == stop_ref.stop_proof(orc, log_n, log_b, q, h, K, coset, D, 5).data


SETTINGS = [   # (log_n, log_b, q, hash, K, coset, D, c, grind)
    (4, 1, 1, 0, 1, False, 0, 1, 0), (4, 1, 3, 1, 2, True, 0, 3, 0), (4, 1, 2, 2, 1, False, 1, 8, 4),
    (6, 3, 3, 0, 1, False, 0, 4, 0), (6, 3, 3, 1, 3, True, 2, 2, 4), (6, 3, 1, 2, 2, False, 2, 8, 0), (6, 3, 2, 2, 3, True, 0, 5, 0),
    (10, 3, 3, 0, 3, True, 4, 4, 4),
]


@pytest.mark.parametrize("s", SETTINGS, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_cpu_verifier_accepts_reference_proofs(zk, orc, s):
    lib = zk.load()
    log_n, log_b, q, h, K, coset, D, c, g = s
    ref = cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, g)
    assert len(ref.data) == lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, c)
    for state in (None, ref.state):
        assert cap_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c) == 0
        assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c) == 0
    # a proof of another cap: -1 by length, strict or not
    for other in {0, 1, 2, 8} - {c}:
        if lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, other) == len(ref.data):
            continue                                        # the clamps make small shapes coincide
        for state in (None, ref.state):
            assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, other) == -1
            assert cap_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, other) == -1


def _kind(name):
    return re.sub(r"\d+", "", name)


def _landed_of(name, ref, K, D, log_n):
    """(tree id, entry) of a cap region."""
    m = re.fullmatch(r"(f_root|root(\d+))\.e(\d+)", name)
    if not m:
        return None
    if m.group(1) == "f_root":
        return 0, int(m.group(3))
    ids = sorted(t for t in ref.c.trees if t >= 1)
    return ids[int(m.group(2))], int(m.group(3))


CORPUS = [   # (log_n, log_b, q, hash, K, coset, D, c, grind): (4,1), (6,3) and (10,3)
    (4, 1, 1, 0, 1, False, 0, 1, 0), (4, 1, 2, 1, 2, True, 1, 2, 3),
    (6, 3, 3, 0, 1, False, 0, 4, 0), (6, 3, 3, 1, 3, True, 2, 3, 4), (6, 3, 3, 2, 2, False, 0, 2, 0),
    (10, 3, 3, 0, 3, True, 4, 4, 4), (10, 3, 3, 0, 1, False, 0, 8, 0),
]


@pytest.mark.parametrize("s", CORPUS, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_tampered_proofs_get_the_reference_check_number(zk, orc, s):
    """One byte flipped in the first region of every kind, in a cap entry a path lands in and in one no path lands in: the library's
    number is the reference's, strict and not; an entry nobody lands in passes the non-strict verification and fails the strict one."""
    lib = zk.load()
    log_n, log_b, q, h, K, coset, D, c, g = s
    ref = cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c, g)
    regs = cap_ref.regions(log_n, log_b, q, g, K, coset, D, c)
    picks, seen, hit, miss = [], set(), None, None
    for name, off, n in regs:
        where = _landed_of(name, ref, K, D, log_n)
        if where is not None:
            landed = where[1] in ref.landed[where[0]]
            if landed and hit is None:
                hit = (name, off, n)
            if not landed and miss is None:
                miss = (name, off, n)
            continue
        if _kind(name) not in seen:
            seen.add(_kind(name))
            picks.append((name, off, n))
    assert hit is not None
    if (log_n, log_b) != (4, 1):
        assert miss is not None                             # a larger shape always has an entry no path of q = 3 queries reaches
    rejected = 0
    for name, off, n in picks + [hit] + ([miss] if miss else []):
        bad = bytearray(ref.data)
        bad[off + n // 2] ^= 0x20
        bad = bytes(bad)
        for state in (None, ref.state):
            want = cap_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c)
            got = _check(lib, bad, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c)
            assert got == want, (name, state is not None, got, want)
            rejected += want != 0
            if (name, off, n) == miss:
                assert (want == 0) == (state is None), (name, want)   # only the transcript replay sees it
            if (name, off, n) == hit:
                assert want != 0, name
    assert rejected >= len(picks)
    # truncated and extended: -1 by length with c > 0, strict or not
    for bad in (ref.data[:-4], ref.data + bytes(4)):
        for state in (None, ref.state):
            assert _check(lib, bad, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c) == -1
            assert cap_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, h, q, g, K, coset, D, c) == -1


def test_cap0_is_zk_verify_stop(zk, orc):
    lib = zk.load()
    ref = stop_ref.stop_proof(orc, 6, 3, 3, 1, 2, True, 2, 4)
    for bad_at in (None, 5, 40, len(ref.data) - 7):
        data = bytearray(ref.data)
        if bad_at is not None:
            data[bad_at] ^= 1
        data = bytes(data)
        for state in (None, ref.state):
            out = C.c_int32(777)
            lib.zk_verify_stop(data, len(data), state, 6, 3, ref.public_last, 1, 3, 4, 2, 1, 2, C.byref(out))
            assert _check(lib, data, state, 6, 3, ref.public_last, 1, 3, 4, 2, True, 2, 0) == out.value


def test_refusals(zk):
    lib = zk.load()
    assert lib.zk_ctx_set_merkle_cap(None, 2) != 0
    assert lib.zk_ctx_get_merkle_cap(None) == 0
    out = C.c_int32(0)
    data = bytes(64)
    assert lib.zk_verify_cap(data, len(data), None, 6, 3, 0, 0, 1, 0, 1, 0, 0, 9, C.byref(out)) == -1    # ZK_ERR_INVALID: cap_log 9
    assert lib.zk_verify_cap(None, 0, None, 6, 3, 0, 0, 1, 0, 1, 0, 0, 2, C.byref(out)) == -1
    assert lib.zk_verify_cap(data, len(data), None, 6, 3, 0, 0, 1, 0, 1, 0, 0, 2, None) == -1
    assert lib.zk_ctx_merkle_cap(None, 0, None, 0) != 0


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", [s for s in __import__("verify_cap_corpus").SHAPES if s[0] <= 6], ids=lambda s: "-".join(str(int(v)) for v in s))
def test_verifier_corpus_gets_the_reference_numbers(zk, orc, shape, hash_kind):
    """The corpus the batched verifier is held to (tests/verify_cap_corpus.py), at its small shapes: zk_verify_cap's number is the
    plain-Python verifier's for every item, strict and not."""
    import verify_cap_corpus
    log_n, log_b, q, g, K, coset, D, c = shape
    items = verify_cap_corpus.corpus(orc, log_n, log_b, q, g, K, coset, D, c, hash_kind)
    assert len(items) > 100
    for strict in (True, False):
        got = verify_cap_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, g, K, coset, D, c, hash_kind, strict)
        for it, n in zip(items, got):
            want = cap_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last & 0xFFFFFFFF, hash_kind, q, g, K, coset, D, c)
            assert n == want, (it.label, strict, int(n), want)
        assert len(set(got.tolist())) > 8
