"""BLAKE2s-256 as a Merkle hash (ZK_HASH_BLAKE2S = 2) without a GPU: the host side of csrc/blake2s.hpp against
hashlib.blake2s -- roots from paths and from coset leaves, the CPU verifier on whole proofs built by tests/blake2s_ref.py in every
setting, the check number it stops at under a wrong hash or a flipped byte -- and the entry points that do not take the hash yet.
Every comparison is for equality.  (The trees of zk_merkle_build_host_ex are built on the device: tests/test_gpu_blake2s.py.)"""
import ctypes as C
import itertools
import os

import pytest

import blake2s_ref
import stop_ref

P = blake2s_ref.P
KIND = blake2s_ref.HASH_KIND
SHAPES = [((4, 1), 2), ((10, 3), 3)]          # (log_n, log_b), the early stop D > 0 tried there


def _check(lib, data, state, log_n, log_b, last, h, q, g, K, coset, D):
    out = C.c_int32(12345)
    rc = lib.zk_verify_stop(data, len(data), state, log_n, log_b, last & 0xFFFFFFFF, h, q, g, K, int(coset), D, C.byref(out))
    assert rc == (0 if out.value == 0 else -6), (rc, out.value, lib.zk_last_error())
    return out.value


# ---- roots from paths ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plen", [0, 1, 2, 13])
def test_root_from_path_and_coset_against_hashlib(zk, plen):
    lib = zk.load()
    rnd = os.urandom(32 * plen)
    pth = [rnd[32 * i:32 * i + 32] for i in range(plen)]
    full = (1 << plen) - 1
    indices = sorted({0, full, 0x1555 & full, 0x0AAA & full})       # both parities at every level
    elements = [0, 1, P - 1, 0xFFFFFFFF]
    for s in (1, 2, 4, 8):
        for first in elements:
            slots = [first] + [elements[(u * 3 + s) % 4] for u in range(1, s)]
            arr = (C.c_uint32 * s)(*slots)
            for idx in indices:
                want = blake2s_ref.root_from_leaf(slots, idx, pth)
                out = C.create_string_buffer(32)
                assert lib.zk_compute_root_from_coset(arr, s, idx, rnd if plen else None, plen, out, KIND) == 0, lib.zk_last_error()
                assert out.raw == want, (s, slots, idx, plen)
                assert zk.compute_root_from_coset(slots, idx, pth, hash="blake2s") == want
                if s == 1:
                    out = C.create_string_buffer(32)
                    assert lib.zk_compute_root_from_path_ex(first, idx, rnd if plen else None, plen, out, KIND) == 0, lib.zk_last_error()
                    assert out.raw == want, (first, idx, plen)
                    assert zk.compute_root_from_path(first, idx, pth, hash="blake2s") == want
    # a leaf alone is its own root: the digest bytes are hashlib's, byte for byte
    if plen == 0:
        import hashlib
        import struct
        assert zk.compute_root_from_path(0x01020304, 0, [], hash="blake2s") == hashlib.blake2s(struct.pack(">I", 0x01020304)).digest()


def test_unknown_kinds_are_still_refused(zk):
    lib = zk.load()
    out = C.create_string_buffer(32)
    arr = (C.c_uint32 * 1)(5)
    for kind in (-1, 3):
        assert lib.zk_compute_root_from_path_ex(5, 0, None, 0, out, kind) == -1
        assert lib.zk_compute_root_from_coset(arr, 1, 0, None, 0, out, kind) == -1


# ---- whole proofs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,stop", SHAPES, ids=["4-1", "10-3"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("coset", [False, True], ids=["values", "cosets"])
def test_cpu_verifier_accepts_reference_proofs(zk, orc, shape, stop, K, coset):
    lib = zk.load()
    log_n, log_b = shape
    for D, q, bits in itertools.product((0, stop), (1, 3), (0, 8)):
        ref = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D, bits)
        assert len(ref.data) == stop_ref.proof_len(log_n, log_b, q, bits, K, coset, D) == lib.zk_proof_data_len_stop(log_n, log_b, q, bits, K, int(coset), D)
        assert blake2s_ref.verify(orc, ref.data, ref.state, log_n, log_b, ref.public_last, KIND, q, bits, K, coset, D) == 0   # the model agrees with itself
        for state in (None, ref.state):
            assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, KIND, q, bits, K, coset, D) == 0, (D, q, bits, state is not None)
        pr = zk.Proof(ref.state, ref.data, log_n, log_b, ref.public_last, "blake2s", q, bits, K, coset, D)
        pr.verify()
        pr.verify(strict=True)
        assert pr.check(strict=True) == 0


@pytest.mark.parametrize("K,coset,D", [(1, False, 0), (2, True, 0), (3, True, 2), (2, False, 2)])
def test_wrong_hash_stops_at_the_models_check(zk, orc, K, coset, D):
    lib = zk.load()
    log_n, log_b, q = 4, 1, 3
    b2 = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D)
    sha = stop_ref.stop_proof(orc, log_n, log_b, q, 0, K, coset, D)
    for ref, kinds in ((b2, (0, 1)), (sha, (KIND,))):
        for kind in kinds:
            for state in (None, ref.state):
                want = blake2s_ref.verify(orc, ref.data, state, log_n, log_b, ref.public_last, kind, q, 0, K, coset, D)
                assert want != 0
                assert _check(lib, ref.data, state, log_n, log_b, ref.public_last, kind, q, 0, K, coset, D) == want, (kind, state is not None)
    # the transcript does not depend on the Merkle hash: a strict check of the SHA-256 proof under BLAKE2s passes the replay and fails
    # at the first path
    assert blake2s_ref.verify(orc, sha.data, sha.state, log_n, log_b, sha.public_last, KIND, q, 0, K, coset, D) == -4


@pytest.mark.parametrize("K,coset,D,bits", [(1, False, 0, 0), (2, True, 0, 8), (3, True, 2, 0), (2, False, 2, 8)])
def test_one_flipped_byte_gives_the_models_check(zk, orc, K, coset, D, bits):
    lib = zk.load()
    log_n, log_b, q = 4, 1, 3
    ref = blake2s_ref.proof(orc, log_n, log_b, q, K, coset, D, bits)
    L = log_n + log_b
    last_path = len(ref.data) - 7                           # inside the last group's last path of the last query
    places = {"f_root": 3, "root0": 32 + 12 + 9, "leaf value": ref.queries_at + 1, "f path": ref.queries_at + 12 + 32 * (L - 1) + 5,
              "second query's value": ref.queries_at + (len(ref.data) - ref.queries_at) // q, "last path": last_path}
    seen = set()
    for name, at in places.items():
        bad = bytearray(ref.data)
        bad[at] ^= 0x40
        bad = bytes(bad)
        for state in (None, ref.state):
            want = blake2s_ref.verify(orc, bad, state, log_n, log_b, ref.public_last, KIND, q, bits, K, coset, D)
            assert want != 0, name
            assert _check(lib, bad, state, log_n, log_b, ref.public_last, KIND, q, bits, K, coset, D) == want, (name, state is not None)
            seen.add(want)
    assert len(seen) >= 4, seen                             # roots, values and paths fail at different checks


# ---- what does not take the hash yet ------------------------------------------------------------------------------------------
def _refused(lib, rc):
    assert rc == -1, rc
    assert b"BLAKE2s" in lib.zk_last_error(), lib.zk_last_error()


def test_out_of_scope_entry_points_refuse_blake2s_by_name(zk):
    """ZK_ERR_INVALID with a message that names the hash, before a handle or a device pointer is looked at."""
    lib = zk.load()
    # zk_verify_check and zk_verify_fold keep the two hashes they were defined with: zk_verify_stop is the verifier of BLAKE2s proofs
    out = C.c_int32(777)
    _refused(lib, lib.zk_verify_check(bytes(100), 100, None, 5, 2, 0, KIND, 1, C.byref(out)))
    _refused(lib, lib.zk_verify_fold(bytes(100), 100, None, 5, 2, 0, KIND, 1, 0, 2, C.byref(out)))
    assert out.value == 777
    _refused(lib, lib.zk_batch_set_hash(None, KIND))
    _refused(lib, lib.zk_verifier_set_hash(None, KIND))
    _refused(lib, lib.zk_shard_set_hash(None, KIND))
    _refused(lib, lib.zk_tail_run(None, None, None, None, KIND, None, None, None))
    root = C.create_string_buffer(32)
    _refused(lib, lib.zk_dev_merkle_build_interleaved(None, 1, 3, None, None, KIND))
    _refused(lib, lib.zk_dev_merkle_commit(None, None, 0, 4, None, None, KIND, root))
    _refused(lib, lib.zk_dev_merkle_commit_finish(None, None, 4, 1, None, KIND, root))
    _refused(lib, lib.zk_dev_merkle_build_chunk(None, 0, 3, None, 4, 0, None, KIND))
    _refused(lib, lib.zk_dev_merkle_finish(None, 4, 1, None, KIND))
    # the same calls with a hash these entry points do take get past the hash check (and then miss their handle)
    assert lib.zk_batch_set_hash(None, 1) == -1 and b"BLAKE2s" not in lib.zk_last_error()


def test_python_classes_without_blake2s_raise(zk):
    assert zk.host.HASHES["blake2s"] == KIND
    with pytest.raises(ValueError, match="blake2s"):
        zk.BatchContext(4, 1, 1, hash="blake2s")
    with pytest.raises(ValueError, match="blake2s"):
        zk.Verifier(4, 1, hash="blake2s")
    with pytest.raises(ValueError, match="blake2s"):
        zk.ShardContext(4, 1, 0, 1, hash="blake2s")
