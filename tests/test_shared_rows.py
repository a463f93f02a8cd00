"""Shared proofs with row leaves without a GPU (zk_verify_shared_rows, zk_proof_data_len_shared_rows, zk_row_leaf_hash):
the row leaf hash against hashlib and the Python chain, the length over the admissible grid, the CPU verifier against the plain-Python
one of tests/rows_ref.py -- accepted model proofs and, for one bit flipped in every region, the same check number -- swapped rows and
public inputs, proofs of the other format, the refusals, and row_leaves = 0 on a corpus of tests/shared_ref.py."""
import ctypes as C

import numpy as np
import pytest

import rows_ref
import shared_ref
import stop_ref

ERR_INVALID, ERR_VERIFY = -1, -6
HASH_NAMES = {0: "sha256", 1: "field"}


def _check(lib, data, state, log_n, log_b, last, lb, h, q, g, K, coset, D, c, rows=1):
    out = C.c_int32(12345)
    arr = np.ascontiguousarray(last, dtype=np.uint32)
    rc = lib.zk_verify_shared_rows(data, len(data), state, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, h, q, g, K, int(coset), D, c, rows, C.byref(out))
    assert rc == (0 if out.value == 0 else ERR_VERIFY), (rc, out.value)
    return out.value


@pytest.mark.parametrize("h", [0, 1])
def test_row_leaf_hash_is_the_model(zk, orc, h):
    """M = 1 .. 256: one compression up to 8 values, the multi-block message / the chain from 16 on; also the tree's own leaf for M <= 8."""
    lib = zk.load()
    rng = np.random.default_rng(20 + h)
    out = np.zeros(32, dtype=np.uint8)
    for lb in range(0, 9):
        m = 1 << lb
        for vals in (rng.integers(0, rows_ref.P, m, dtype=np.uint64).astype(np.uint32), np.full(m, rows_ref.P - 1, dtype=np.uint32),
                     np.zeros(m, dtype=np.uint32)):
            assert lib.zk_row_leaf_hash(vals.ctypes.data_as(C.c_void_p), m, h, out.ctypes.data_as(C.c_void_p)) == 0
            want = rows_ref.row_leaf_hash(orc, list(vals), h)
            assert out.tobytes() == want, (m, h)
            if m <= 8:                                          # ... which is the existing coset leaf
                assert zk.host.compute_root_from_coset(vals, 0, [], hash=HASH_NAMES[h]) == want
    vals = np.zeros(512, dtype=np.uint32)
    for m, kind in ((0, 0), (3, 0), (12, 1), (512, 0), (16, 2), (16, 7)):
        assert lib.zk_row_leaf_hash(vals.ctypes.data_as(C.c_void_p), m, kind, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID
    assert lib.zk_row_leaf_hash(None, 16, 0, out.ctypes.data_as(C.c_void_p)) == ERR_INVALID


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
                                    got = lib.zk_proof_data_len_shared_rows(log_n, log_b, q, 0, K, coset, D, c, lb, 1)
                                    off = lib.zk_proof_data_len_shared_rows(log_n, log_b, q, 0, K, coset, D, c, lb, 0)
                                    assert off == lib.zk_proof_data_len_shared(log_n, log_b, q, 0, K, coset, D, c, lb)
                                    if not ok or lb > 8 or lb == 0:
                                        assert got == 0, (log_n, log_b, q, K, coset, D, c, lb)
                                    else:
                                        assert got == rows_ref.proof_len(log_n, log_b, q, 0, K, coset, D, c, lb), (log_n, log_b, q, K, coset, D, c, lb)
                                        assert got == lib.zk_proof_data_len_cap(log_n, log_b, q, 0, K, coset, D, c) + 12 * ((1 << lb) - 1) * (1 + q)
                                        n += 1
    assert n > 20000
    assert lib.zk_proof_data_len_shared_rows(10, 3, 3, 5, 2, 1, 2, 4, 3, 1) == rows_ref.proof_len(10, 3, 3, 5, 2, True, 2, 4, 3)   # grinding: 8 bytes
    assert lib.zk_proof_data_len_shared_rows(10, 3, 1, 0, 4, 0, 0, 2, 3, 1) == 0 and lib.zk_proof_data_len_shared_rows(10, 3, 1, 0, 1, 0, 0, 9, 3, 1) == 0
    # the point of the format: 64 x 2^20 at 32 queries
    assert lib.zk_proof_data_len_shared(17, 3, 32, 0, 1, 0, 0, 0, 6) - lib.zk_proof_data_len_shared_rows(17, 3, 32, 0, 1, 0, 0, 0, 6, 1) == \
        32 * 63 * (3 * (12 + 32 * 20) - 12) + 32 * 63


# (log_n, log_b, lb, K, coset, D, c, q, hash)
SHAPES = [(2, 1, 1, 1, False, 0, 8, 1, 0),       # L = 3, ce_f = 2: paths of one digest
          (2, 1, 4, 1, False, 0, 8, 2, 1),
          (4, 1, 3, 2, True, 1, 0, 2, 0),
          (5, 2, 3, 3, True, 2, 3, 3, 1),        # one compression per row (lb <= 3), K = 3 with coset leaves and an early stop
          (5, 2, 4, 3, True, 2, 2, 2, 0),        # two SHA-256 blocks per row
          (4, 2, 4, 1, False, 0, 2, 2, 1),       # a chain of two field compressions
          (4, 1, 8, 2, False, 0, 1, 1, 0),       # 256 statements: 16 data blocks and the padding block
          (4, 1, 8, 1, True, 0, 0, 1, 1)]        # ... a chain of 32


def _ids(s):
    return "-".join(str(int(v)) for v in s)


@pytest.mark.parametrize("s", SHAPES, ids=_ids)
def test_cpu_verifier_accepts_model_proofs(zk, orc, s):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    assert len(ref.data) == lib.zk_proof_data_len_shared_rows(log_n, log_b, q, 0, K, int(coset), D, c, lb, 1)
    for state in (None, ref.state):
        assert rows_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == 0
        assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == 0
    sp = zk.SharedProof(ref.state, ref.data, log_n, log_b, lb, ref.public_last, HASH_NAMES[h], q, 0, K, coset, D, c, shared_rows=True)
    assert sp.expected_len() == len(ref.data) and sp.check(strict=True) == 0 and sp.check() == 0
    sp.verify(strict=True)


def test_grinding_is_replayed(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h, g = 4, 1, 2, 1, False, 0, 1, 2, 0, 6
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, g)
    assert ref.nonce is not None
    for state in (None, ref.state):
        assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c) == 0
    regs = {name: (off, n) for name, off, n in rows_ref.regions(log_n, log_b, q, g, K, coset, D, c, lb)}
    bad = bytearray(ref.data)
    bad[regs["nonce"][0]] ^= 1
    want = rows_ref.verify(orc, bytes(bad), ref.state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c)
    assert _check(lib, bytes(bad), ref.state, log_n, log_b, ref.public_last, lb, h, q, g, K, coset, D, c) == want != 0


@pytest.mark.parametrize("s", [SHAPES[3], SHAPES[5]], ids=_ids)
def test_one_bit_in_every_region(zk, orc, s):
    """Every cap entry, every alpha, every value, the count and the path of every row, every other field: one bit flipped, and the library's
    number is the plain-Python verifier's, strict and not.  One proof with lb <= 3, one with lb >= 4."""
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    regs = rows_ref.regions(log_n, log_b, q, 0, K, coset, D, c, lb)
    assert len(regs) > 100
    seen, rejected = set(), 0
    for name, off, n in regs:
        bad = bytearray(ref.data)
        bad[off + n // 2] ^= 0x20
        bad = bytes(bad)
        for state in (None, ref.state):
            want = rows_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c)
            got = _check(lib, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c)
            assert got == want, (name, state is not None, got, want)
            if state is not None:
                assert want != 0, name                      # the replay sees every byte
                rejected += 1
            seen.add(want)
    assert rejected == len(regs)
    assert {-1, -2, -4, -5, -6}.issubset(seen) and any(w <= -1000 for w in seen) and any(-200 > w > -400 for w in seen), sorted(seen)
    for bad in (ref.data[:-4], ref.data + bytes(4)):
        for state in (None, ref.state):
            assert _check(lib, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -1
            assert rows_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -1


@pytest.mark.parametrize("s", [SHAPES[3], SHAPES[5]], ids=_ids)
def test_swapped_rows_and_public_inputs(zk, orc, s):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = s
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    regs = {name: (off, n) for name, off, n in rows_ref.regions(log_n, log_b, q, 0, K, coset, D, c, lb)}
    d = ref.data
    # two values of one row trade places: the sum over the statements changes
    for i in range(3):
        v0, v1 = regs[f"q0.row{i}.value0"][0], regs[f"q0.row{i}.value1"][0]
        assert d[v0:v0 + 4] != d[v1:v1 + 4]
        bad = bytearray(d)
        bad[v0:v0 + 4], bad[v1:v1 + 4] = d[v1:v1 + 4], d[v0:v0 + 4]
        assert _check(lib, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -2
        assert rows_ref.verify(orc, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -2
    # statements 0 and 1 trade places everywhere -- alphas, public inputs, their values in all three rows of every query: the sum is
    # the same sum, and the leaf, which holds the row in statement order, no longer climbs to the cap: -4 (without the replay, which
    # would stop at the traded alphas)
    bad, last = bytearray(d), list(ref.public_last)
    last[0], last[1] = last[1], last[0]
    pairs = [(regs["s0.alpha0"][0], regs["s1.alpha0"][0], 12)]
    pairs += [(regs[f"q{k}.row{i}.value0"][0], regs[f"q{k}.row{i}.value1"][0], 4) for k in range(q) for i in range(3)]
    for a, b, n in pairs:
        bad[a:a + n], bad[b:b + n] = d[b:b + n], d[a:a + n]
    assert _check(lib, bytes(bad), None, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -4
    assert rows_ref.verify(orc, bytes(bad), None, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -4
    assert _check(lib, bytes(bad), ref.state, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) <= -1000
    # the same trade in the rows x + B and x + 2B only (row x and the alphas as sent) cannot keep the sum; a changed digest in the path
    # of a row is that row's number
    for i in range(3):
        bad = bytearray(d)
        bad[regs[f"q0.row{i}.path"][0] + 5] ^= 1
        assert _check(lib, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -(4 + i)
        assert rows_ref.verify(orc, bytes(bad), None, log_n, log_b, ref.public_last, lb, h, q, 0, K, coset, D, c) == -(4 + i)
    last = list(ref.public_last)
    assert last[0] != last[1]
    last[0], last[1] = last[1], last[0]
    for state in (None, ref.state):
        assert _check(lib, ref.data, state, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -2
        assert rows_ref.verify(orc, ref.data, state, log_n, log_b, last, lb, h, q, 0, K, coset, D, c) == -2


def test_other_format_and_refusals(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, h = 4, 2, 2, 1, False, 0, 2, 2, 0
    rows = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    plain = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
    assert rows.public_last == plain.public_last and len(rows.data) < len(plain.data)
    arr = np.array(list(rows.public_last) * 64, dtype=np.uint32)
    ptr = arr.ctypes.data_as(C.c_void_p)
    for strict in (False, True):
        # a rows proof read as a plain shared proof, and the other way round: -1
        out = C.c_int32(7)
        assert lib.zk_verify_shared(rows.data, len(rows.data), rows.state if strict else None, log_n, log_b, ptr, lb, h, q, 0, K, int(coset), D, c, C.byref(out)) == ERR_VERIFY
        assert out.value == -1
        assert _check(lib, plain.data, plain.state if strict else None, log_n, log_b, arr, lb, h, q, 0, K, coset, D, c, 1) == -1
        assert rows_ref.verify(orc, plain.data, plain.state if strict else None, log_n, log_b, rows.public_last, lb, h, q, 0, K, coset, D, c) == -1
        assert _check(lib, plain.data, plain.state if strict else None, log_n, log_b, arr, lb, h, q, 0, K, coset, D, c, 0) == 0
        for other in (1, 3, 8):
            assert _check(lib, rows.data, rows.state if strict else None, log_n, log_b, arr, other, h, q, 0, K, coset, D, c) == -1
    # rows with lb = 0 or 9, and rows with BLAKE2s: check -1, ZK_ERR_INVALID
    for bad_lb, kind in ((0, h), (9, h), (lb, 2)):
        out = C.c_int32(777)
        rc = lib.zk_verify_shared_rows(rows.data, len(rows.data), None, log_n, log_b, ptr, bad_lb, kind, q, 0, K, int(coset), D, c, 1, C.byref(out))
        assert (rc, out.value) == (ERR_INVALID, -1), (bad_lb, kind)
        assert rows_ref.verify(orc, rows.data, None, log_n, log_b, list(arr), bad_lb, kind, q, 0, K, coset, D, c) == -1
    assert lib.zk_proof_data_len_shared_rows(log_n, log_b, q, 0, K, int(coset), D, c, 0, 1) == 0
    out = C.c_int32(0)
    assert lib.zk_verify_shared_rows(None, 0, None, log_n, log_b, ptr, lb, h, q, 0, K, int(coset), D, c, 1, C.byref(out)) == ERR_INVALID
    assert lib.zk_verify_shared_rows(rows.data, len(rows.data), None, log_n, log_b, None, lb, h, q, 0, K, int(coset), D, c, 1, C.byref(out)) == ERR_INVALID
    assert lib.zk_verify_shared_rows(rows.data, len(rows.data), None, log_n, log_b, ptr, lb, h, q, 0, K, int(coset), D, c, 1, None) == ERR_INVALID
    assert lib.zk_verify_shared_rows(rows.data, len(rows.data), None, log_n, log_b, ptr, lb, 7, q, 0, K, int(coset), D, c, 1, C.byref(out)) == ERR_INVALID
    assert lib.zk_batch_set_shared_rows(None, 1) == ERR_INVALID and lib.zk_batch_get_shared_rows(None) == 0
    assert lib.zk_dev_merkle_build_rows(None, 3, 1, None, None, 0) == ERR_INVALID


def test_rows_off_is_zk_verify_shared(zk, orc):
    """zk_verify_shared_rows(.., 0, ..) on shared_ref's proofs, valid and with one bit flipped in a spread of regions: the number, the return
    code and the message of zk_verify_shared."""
    lib = zk.load()
    for s in ((5, 2, 3, 3, True, 2, 3, 3, 1), (6, 3, 2, 1, False, 0, 2, 2, 0), (2, 1, 1, 1, False, 0, 0, 1, 2)):
        log_n, log_b, lb, K, coset, D, c, q, h = s
        ref = shared_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c)
        regs = shared_ref.regions(log_n, log_b, q, 0, K, coset, D, c, lb)
        arr = np.ascontiguousarray(ref.public_last, dtype=np.uint32)
        ptr = arr.ctypes.data_as(C.c_void_p)
        corpus = [ref.data, ref.data[:-1], ref.data + b"\0"]
        for name, off, n in regs[::max(1, len(regs) // 40)]:
            bad = bytearray(ref.data)
            bad[off + n // 2] ^= 0x20
            corpus.append(bytes(bad))
        numbers = set()
        for data in corpus:
            for state in (None, ref.state):
                a, b = C.c_int32(1), C.c_int32(2)
                ra = lib.zk_verify_shared(data, len(data), state, log_n, log_b, ptr, lb, h, q, 0, K, int(coset), D, c, C.byref(a))
                ea = lib.zk_last_error()
                rb = lib.zk_verify_shared_rows(data, len(data), state, log_n, log_b, ptr, lb, h, q, 0, K, int(coset), D, c, 0, C.byref(b))
                assert (ra, a.value) == (rb, b.value) and (ra == 0 or ea == lib.zk_last_error())
                numbers.add(a.value)
        assert 0 in numbers and len(numbers) > 3, numbers
        for bad_lb in (0, 9):
            a, b = C.c_int32(1), C.c_int32(2)
            ra = lib.zk_verify_shared(ref.data, len(ref.data), None, log_n, log_b, ptr, bad_lb, h, q, 0, K, int(coset), D, c, C.byref(a))
            rb = lib.zk_verify_shared_rows(ref.data, len(ref.data), None, log_n, log_b, ptr, bad_lb, h, q, 0, K, int(coset), D, c, 0, C.byref(b))
            assert (ra, a.value) == (rb, b.value) == (ERR_INVALID, -1)
