"""Shared proofs without a GPU (zk_verify_shared, zk_proof_data_len_shared): the length against tests/shared_ref.py over
the admissible grid, the CPU verifier against the plain-Python one -- accepted model proofs and, for one bit flipped in every region, the
same check number -- swapped public inputs, proofs of another width, the refusals, and the older entry points on their own corpora."""
import ctypes as C
import struct

import numpy as np
import pytest

import cap_ref
import shared_ref
import stop_ref

ERR_INVALID, ERR_VERIFY = -1, -6


def _check(lib, data, state, log_n, log_b, last, lb, h, q, g, K, coset, D, c):
    out = C.c_int32(12345)
    arr = np.ascontiguousarray(last, dtype=np.uint32)
    rc = lib.zk_verify_shared(data, len(data), state, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, h, q, g, K, int(coset), D, c, C.byref(out))
    assert rc == (0 if out.value == 0 else ERR_VERIFY), (rc, out.value)
    return out.value


def test_proof_length_grid(zk):
    lib = zk.load()
    n = 0
    for log_n in (2, 3, 5, 8, 12):
        for log_b in (1, 3, 5):
            for q in (1, 3, 16):
                for K in (1, 2, 3):
                    for coset in (0, 1):
                        for D in (0, 1, 2, 5, 8, 9):
                            ok = stop_ref.admissible(log_n, log_b, D)
                            for c in range(0, 9):
                                for lb in range(0, 10):
                                    got = lib.zk_proof_data_len_shared(log_n, log_b, q, 0, K, coset, D, c, lb)
                                    if not ok or lb > 8:
                                        assert got == 0, (log_n, log_b, q, K, coset, D, c, lb)
                                    elif lb == 0:
                                        assert got == lib.zk_proof_data_len_cap(log_n, log_b, q, 0, K, coset, D, c) != 0
                                    else:
                                        assert got == shared_ref.proof_len(log_n, log_b, q, 0, K, coset, D, c, lb), (log_n, log_b, q, K, coset, D, c, lb)
                                        n += 1
    assert n > 20000
    assert lib.zk_proof_data_len_shared(10, 3, 3, 5, 2, 1, 2, 4, 3) == shared_ref.proof_len(10, 3, 3, 5, 2, True, 2, 4, 3)   # grinding: 8 bytes
    assert lib.zk_proof_data_len_shared(10, 3, 1, 0, 4, 0, 0, 2, 3) == 0 and lib.zk_proof_data_len_shared(10, 3, 1, 0, 1, 0, 0, 9, 3) == 0


# (log_n, log_b, lb, K, coset, D, c, q, hash)
SHAPES = [(2, 1, 1, 1, False, 0, 0, 1, 0), (4, 1, 1, 2, True, 1, 8, 2, 0), (5, 2, 3, 3, True, 2, 3, 3, 1), (6, 3, 2, 1, False, 0, 2, 2, 0),
          (10, 3, 2, 2, False, 4, 0, 1, 0)]


def _ids(s):
    return "-".join(str(int(v)) for v in s)


@pytest.mark.parametrize("s", SHAPES, ids=_ids)
def test_cpu_verifier_accepts_model_proofs(zk, orc, s):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    assert len(ref.data) == lib.zk_proof_data_len_shared(log_n, log_b, q, 0, K, int(coset), D, c, lb)
    for state in (None, ref.state):
        assert shared_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == 0
        assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == 0
    sp = zk.SharedProof(ref.state, ref.data, log_n, log_b, lb, ref.public_last, {0: "sha256", 1: "field"}[h], q, 0, K, coset, D, c)
    assert sp.expected_len() == len(ref.data) and sp.check(strict=True) == 0 and sp.check() == 0
    sp.verify(strict=True)


def test_grinding_is_replayed(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h, g = 4, 1, 2, 1, False, 0, 1, 2, 0, 6
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, g)
    assert ref.nonce is not None
    for state in (None, ref.state):
        assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c) == 0
    regs = {name: (off, n) for name, off, n in shared_ref.regions(log_n, log_b, q, g, K, coset, D, c, lb)}
    bad = bytearray(ref.data)
    bad[regs["nonce"][0]] ^= 1
    want = shared_ref.verify(orc, bytes(bad), ref.state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c)
    assert _check(lib, bytes(bad), ref.state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c) == want != 0


@pytest.mark.parametrize("s", [SHAPES[2], SHAPES[3]], ids=_ids)
def test_one_bit_in_every_region(zk, orc, s):
    """Every cap entry, every alpha, every f value, count and path of every statement, every other field: one bit flipped, and the
    library's number is the plain-Python verifier's, strict and not."""
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    regs = shared_ref.regions(log_n, log_b, q, 0, K, coset, D, c, lb)
    assert len(regs) > 100
    seen, rejected = set(), 0
    for name, off, n in regs:
        bad = bytearray(ref.data)
        bad[off + n // 2] ^= 0x20
        bad = bytes(bad)
        for state in (None, ref.state):
            want = shared_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c)
            got = _check(lib, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c)
            assert got == want, (name, state is not None, got, want)
            if state is not None:
                assert want != 0, name                      # the replay sees every byte
                rejected += 1
            seen.add(want)
    assert rejected == len(regs)
    # (bit 5 of a count's byte 4 makes it larger than any path: -1, not -3; test_statement_numbers_follow_wire_order has the -3)
    assert {-1, -2, -4, -5, -6}.issubset(seen) and any(w <= -1000 for w in seen) and any(-200 > w > -400 for w in seen), sorted(seen)
    for bad in (ref.data[:-4], ref.data + bytes(4)):
        for state in (None, ref.state):
            assert _check(lib, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -1
            assert shared_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -1


def test_statement_numbers_follow_wire_order(zk, orc):
    """A path of a later statement is reported only if every earlier tuple holds: -5 of statement 0 wins over -4 of statement 2."""
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = SHAPES[3]
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    regs = {name: (off, n) for name, off, n in shared_ref.regions(log_n, log_b, q, 0, K, coset, D, c, lb)}
    bad = bytearray(ref.data)
    for name in ("q0.s2.f0.path", "q0.s0.f1.path"):
        bad[regs[name][0] + 5] ^= 1
    assert _check(lib, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -5
    assert shared_ref.verify(orc, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -5
    only = bytearray(ref.data)
    only[regs["q0.s2.f0.path"][0] + 5] ^= 1
    assert _check(lib, bytes(only), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -4
    # -3: with the length fixed, a wrong count that still parses has to be paid back at once -- statement 3's f(gx) path gives its last
    # digest to the f(g^2 x) path, whose value moves up with it: every value read before -3 is intact
    c1, p1, v2, p2 = (regs[f"q0.s3.{name}"] for name in ("f1.count", "f1.path", "f2.value", "f2.path"))
    plen = p1[1] // 32
    d = ref.data
    seg = (struct.pack("<Q", plen - 1) + d[p1[0]:p1[0] + 32 * (plen - 1)] + d[v2[0]:v2[0] + 4] + struct.pack("<Q", plen + 1) +
           d[p1[0] + 32 * (plen - 1):p1[0] + 32 * plen] + d[p2[0]:p2[0] + p2[1]])
    moved = d[:c1[0]] + seg + d[p2[0] + p2[1]:]
    assert len(moved) == len(d) and moved != d
    assert _check(lib, moved, None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -3
    assert shared_ref.verify(orc, moved, None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -3


@pytest.mark.parametrize("s", [SHAPES[2], SHAPES[3]], ids=_ids)
def test_swapped_public_inputs(zk, orc, s):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    last = list(ref.public_last)
    assert last[0] != last[1]
    last[0], last[1] = last[1], last[0]
    for state in (None, ref.state):
        assert _check(lib, ref.data, state, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -2
        assert shared_ref.verify(orc, ref.data, state, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -2


def test_other_widths_and_plain_proofs(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = SHAPES[3]
    ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    plain = cap_ref.proof(orc, log_n, log_b, q, h, K, coset, D, c)
    wide = list(ref.public_last) * 64
    for state in (None, ref.state):
        for other in (1, 3, 8):
            assert _check(lib, ref.data, state, log_n, log_b, wide, other, h, q, 0, K, coset, D, c) == -1
            assert shared_ref.verify(orc, ref.data, state, log_n, log_b, wide, other, h, q, 0, K, coset, D, c) == -1
        assert _check(lib, plain.data, state and plain.state, log_n, log_b, wide, lb, h, q, 0, K, coset, D, c) == -1
    # a batch of one is a plain proof, and 2^9 statements are too many: check -1, ZK_ERR_INVALID
    arr = np.array(wide, dtype=np.uint32)
    for bad_lb in (0, 9):
        for data in (ref.data, plain.data):
            out = C.c_int32(777)
            rc = lib.zk_verify_shared(data, len(data), None, log_n, log_b, arr.ctypes.data_as(C.c_void_p), bad_lb, h, q, 0, K, int(coset), D, c, C.byref(out))
            assert (rc, out.value) == (ERR_INVALID, -1)
            assert shared_ref.verify(orc, data, None, log_n, log_b, wide, bad_lb, h, q, 0, K, coset, D, c) == -1
    out = C.c_int32(0)
    assert lib.zk_verify_shared(None, 0, None, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, h, q, 0, K, int(coset), D, c, C.byref(out)) == ERR_INVALID
    assert lib.zk_verify_shared(ref.data, len(ref.data), None, log_n, log_b, None, lb, h, q, 0, K, int(coset), D, c, C.byref(out)) == ERR_INVALID
    assert lib.zk_verify_shared(ref.data, len(ref.data), None, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, h, q, 0, K, int(coset), D, c, None) == ERR_INVALID
    assert lib.zk_verify_shared(ref.data, len(ref.data), None, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, 7, q, 0, K, int(coset), D, c, C.byref(out)) == ERR_INVALID
    assert lib.zk_batch_prove_shared(None, None, 0, None, None) == ERR_INVALID


def test_older_entry_points_answer_as_before(zk, orc):
    """zk_verify_cap and zk_proof_data_len_cap on the inputs of the existing corpora (their modules, unedited): the plain-Python
    verifier's numbers, and the lengths of cap_ref."""
    import test_merkle_cap
    import verify_cap_corpus
    lib = zk.load()
    for log_n, log_b, q, h, K, coset, D, c, g in test_merkle_cap.SETTINGS + test_merkle_cap.CORPUS:
        assert lib.zk_proof_data_len_cap(log_n, log_b, q, g, K, int(coset), D, c) == cap_ref.proof_len(log_n, log_b, q, g, K, coset, D, c)
        assert lib.zk_proof_data_len_shared(log_n, log_b, q, g, K, int(coset), D, c, 0) == cap_ref.proof_len(log_n, log_b, q, g, K, coset, D, c)
    shape = next(s for s in verify_cap_corpus.SHAPES if s[0] <= 6)
    log_n, log_b, q, g, K, coset, D, c = shape
    items = verify_cap_corpus.corpus(orc, log_n, log_b, q, g, K, coset, D, c, 0)
    for strict in (True, False):
        got = verify_cap_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, c, 0, strict)
        for it, n in zip(items, got):
            want = cap_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last & 0xFFFFFFFF, 0, q, g, K, coset, D, c)
            assert n == want, (it.label, strict, int(n), want)
