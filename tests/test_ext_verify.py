"""The CPU verifier of proofs with challenges in E = F_P[u] / (u^2 - 5) (zk_verify_ext, zk_proof_data_len_ext; csrc/transcript.hpp "ext",
DESIGN.md 7j) on proofs tests/ext_ref.py builds without the library: accepted strict and not, the length formula, the model verifier's
check number for a changed byte in every kind of region of the wire format -- the component-1 word of an alpha, of a beta, of the free
term, of a coefficient and of an opened value among them -- and the refusals."""
import ctypes as C
import re

import pytest

import cap_ref
import ext_ref

ERR_INVALID, ERR_VERIFY = -1, -6

# (log_n, log_b, q, hash, K, coset, D, cap, grinding bits): every K x leaf format, D in {0, 2}, cap in {0, 4, 8}, q in {1, 16}, grinding in {0, 8},
# hash in {0, 1} and the three sizes appear (test_the_grid_covers_every_value); D = 2 needs log_n >= 3
SETTINGS = [
    (2, 1, 1, 0, 1, False, 0, 0, 0),
    (2, 1, 16, 1, 2, True, 0, 4, 8),
    (4, 2, 1, 0, 1, True, 0, 4, 0),
    (4, 2, 16, 1, 1, False, 2, 0, 8),
    (4, 2, 1, 1, 2, False, 0, 8, 0),
    (4, 2, 16, 0, 2, True, 2, 4, 0),
    (4, 2, 1, 0, 3, False, 2, 4, 8),
    (4, 2, 16, 0, 3, True, 0, 8, 0),
    (10, 3, 1, 0, 1, False, 0, 4, 0),
    (10, 3, 1, 1, 1, True, 2, 0, 0),
    (10, 3, 1, 0, 2, False, 2, 8, 8),
    (10, 3, 1, 1, 2, True, 0, 0, 0),
    (10, 3, 1, 1, 3, False, 0, 8, 0),
    (10, 3, 1, 0, 3, True, 2, 4, 8),
]
C1_KINDS = ("alpha#.c1", "beta#.c1", "free_term.c1", "coef#.c1", "q#.cp.c1", "q#.g#.value#.c1", "q#.g#.slot#.c1")


def test_the_grid_covers_every_value():
    assert {(s[4], s[5]) for s in SETTINGS} == {(k, c) for k in (1, 2, 3) for c in (False, True)}
    assert {s[6] for s in SETTINGS} == {0, 2} and {s[7] for s in SETTINGS} == {0, 4, 8}
    assert {s[2] for s in SETTINGS} == {1, 16} and {s[8] for s in SETTINGS} == {0, 8} and {s[3] for s in SETTINGS} == {0, 1}
    assert {s[:2] for s in SETTINGS} == {(2, 1), (4, 2), (10, 3)}


def _lib_verify(lib, data, state, log_n, log_b, public_last, hash_kind, q, bits, K, coset, D, c, ext_log=1):
    chk = C.c_int32(77)
    rc = lib.zk_verify_ext(bytes(data), len(data), state, log_n, log_b, public_last, hash_kind, q, bits, K, int(coset), D, c, ext_log, C.byref(chk))
    assert rc == (0 if chk.value == 0 else ERR_VERIFY), (rc, chk.value, lib.zk_last_error())
    return chk.value


def _kind(name):
    return re.sub(r"\d+", "#", name.replace(".c0", ".cZ").replace(".c1", ".cO")).replace(".cZ", ".c0").replace(".cO", ".c1")


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_model_proofs_verify_and_a_changed_byte_gets_the_model_check_number(zk, orc, setting):
    log_n, log_b, q, hash_kind, K, coset, D, c, bits = setting
    lib = zk.load()
    pr = ext_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits)
    args = (log_n, log_b, pr.public_last, hash_kind, q, bits, K, coset, D, c)
    want_len = ext_ref.proof_len(log_n, log_b, q, bits, K, coset, D, c)
    assert lib.zk_proof_data_len_ext(log_n, log_b, q, bits, K, int(coset), D, c, 1) == want_len == len(pr.data)
    assert lib.zk_proof_data_len_ext(log_n, log_b, q, bits, K, int(coset), D, c, 0) == lib.zk_proof_data_len_cap(log_n, log_b, q, bits, K, int(coset), D, c)
    for state in (pr.state, None):
        assert ext_ref.verify(orc, pr.data, state, *args) == 0
        assert _lib_verify(lib, pr.data, state, *args) == 0
    assert _lib_verify(lib, pr.data, bytes(32), *args) == -1999

    # every region of the wire format, a low bit of its first byte (of a cap: its first and last entry); the first region of every kind also a
    # high bit of its last byte
    regs = ext_ref.regions(log_n, log_b, q, bits, K, coset, D, c)
    by_kind = {}
    for r in regs:
        by_kind.setdefault(_kind(r[0]), []).append(r)
    changes = []
    for kind, rs in by_kind.items():
        changes.append((kind, rs[0][0], rs[0][1] + rs[0][2] - 1, 0x80))
        for i, (name, off, n) in enumerate(rs):
            entry = re.search(r"\.e(\d+)$", name)
            if entry and i + 1 < len(rs) and int(entry.group(1)) and rs[i + 1][0].split(".e")[0] == name.split(".e")[0]:
                continue                                                             # an inner entry of a cap
            changes.append((kind, name, off, 1))
    seen = set()
    for kind, name, at, bit in changes:
        bad = bytearray(pr.data)
        bad[at] ^= bit
        for state in (pr.state, None):
            want = ext_ref.verify(orc, bytes(bad), state, *args)
            assert want != 0 or state is None, (name, at)                            # the strict replay misses nothing
            assert _lib_verify(lib, bad, state, *args) == want, (name, at, bit, state is not None)
            if state is None and at == by_kind[kind][0][1]:
                seen.add((kind, want))
    kinds = set(by_kind)
    assert {"alpha#.c1", "beta#.c1"} <= kinds and ("coef#.c1" if D else "free_term.c1") in kinds
    assert ("q#.g#.slot#.c1" if coset else "q#.g#.value#.c1") in kinds and (coset or "q#.cp.c1" in kinds)
    assert all(k in C1_KINDS or not k.endswith(".c1") for k in kinds)
    # without the replay, a changed component-1 word fails the check the component-0 word beside it fails
    for k in kinds:
        if k.endswith(".c1"):
            assert {w for kk, w in seen if kk == k} == {w for kk, w in seen if kk == k[:-1] + "0"}, k

    # truncated, extended, and read as the other format
    for data in (pr.data[:-1], pr.data + b"\0", pr.data[:40]):
        for state in (pr.state, None):
            assert _lib_verify(lib, data, state, *args) == -1
    for state in (pr.state, None):
        assert _lib_verify(lib, pr.data, state, *args, ext_log=0) == -1


@pytest.mark.parametrize("setting", [SETTINGS[2], SETTINGS[6], SETTINGS[9]], ids=lambda s: "-".join(str(int(v)) for v in s))
def test_ext_log_0_is_zk_verify_cap(zk, orc, setting):
    """With ext_log = 0 every input gets zk_verify_cap's answer, and a base-field proof read with ext_log = 1 gets -1."""
    log_n, log_b, q, hash_kind, K, coset, D, c, bits = setting
    lib = zk.load()
    base = cap_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits)
    ext = ext_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits)
    args = (log_n, log_b, base.public_last, hash_kind, q, bits, K, coset, D, c)
    flipped = bytearray(base.data)
    flipped[len(flipped) // 2] ^= 4
    for data in (base.data, bytes(flipped), base.data[:-3], ext.data):
        for state in (base.state, None):
            chk = C.c_int32(55)
            lib.zk_verify_cap(data, len(data), state, log_n, log_b, base.public_last, hash_kind, q, bits, K, int(coset), D, c, C.byref(chk))
            assert _lib_verify(lib, data, state, *args, ext_log=0) == chk.value
    assert _lib_verify(lib, base.data, base.state, *args, ext_log=0) == 0
    for state in (base.state, None):
        assert _lib_verify(lib, base.data, state, *args, ext_log=1) == -1


def test_refusals_name_what_they_refuse(zk, orc):
    lib = zk.load()
    pr = ext_ref.proof(orc, 4, 2, 1, 0, 1, False, 0, 0, 0)
    chk = C.c_int32(55)
    assert lib.zk_verify_ext(pr.data, len(pr.data), pr.state, 4, 2, pr.public_last, 0, 1, 0, 1, 0, 0, 0, 2, C.byref(chk)) == ERR_INVALID
    assert chk.value == -1 and b"ext_log" in lib.zk_last_error() and b"zk_verify_ext" in lib.zk_last_error()
    chk = C.c_int32(55)
    assert lib.zk_verify_ext(pr.data, len(pr.data), pr.state, 4, 2, pr.public_last, 2, 1, 0, 1, 0, 0, 0, 1, C.byref(chk)) == ERR_INVALID
    msg = lib.zk_last_error()
    assert chk.value == -1 and b"ext_log" in msg and b"BLAKE2s" in msg and b"hash 2" in msg
    assert lib.zk_verify_ext(None, 0, None, 4, 2, 0, 0, 1, 0, 1, 0, 0, 0, 1, C.byref(chk)) == ERR_INVALID
    assert lib.zk_verify_ext(pr.data, len(pr.data), None, 4, 2, 0, 0, 1, 0, 1, 0, 0, 0, 1, None) == ERR_INVALID
    assert lib.zk_verify_ext(pr.data, len(pr.data), None, 4, 2, pr.public_last, 0, 1, 0, 4, 0, 0, 0, 1, C.byref(chk)) == ERR_INVALID   # fold_log 4
    assert lib.zk_verify_ext(pr.data, len(pr.data), None, 4, 2, pr.public_last, 0, 1, 0, 1, 0, 0, 9, 1, C.byref(chk)) == ERR_INVALID   # cap_log 9
    for ext_log in (2, 3, 2**31):
        assert lib.zk_proof_data_len_ext(4, 2, 1, 0, 1, 0, 0, 0, ext_log) == 0
    assert lib.zk_proof_data_len_ext(4, 2, 1, 0, 4, 0, 0, 0, 1) == 0 and lib.zk_proof_data_len_ext(4, 2, 1, 0, 1, 0, 9, 0, 1) == 0


def test_proof_objects_carry_ext_log(zk, orc):
    """zkstark_amd.Proof(ext_log=1): verify / check go to zk_verify_ext, the length to zk_proof_data_len_ext."""
    log_n, log_b, q, hash_kind, K, coset, D, c, bits = SETTINGS[5]
    ref = ext_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits)
    kw = dict(log_n=log_n, log_blowup=log_b, public_last=ref.public_last, hash="sha256", queries=q, grind_bits=bits, fold_log=K, coset_leaves=coset,
              stop_log=D, cap_log=c)
    pr = zk.Proof(ref.state, ref.data, ext_log=1, **kw)
    assert pr.expected_len() == len(ref.data)
    pr.verify()
    pr.verify(strict=True)
    assert pr.check(strict=True) == 0 and pr.check() == 0
    assert zk.Proof(ref.state, ref.data, **kw).check() == -1 and zk.Proof(ref.state, ref.data, **kw).ext_log == 0
    bad = bytearray(ref.data)
    bad[len(ref.data) - 5] ^= 1
    want = ext_ref.verify(orc, bytes(bad), None, log_n, log_b, ref.public_last, hash_kind, q, bits, K, coset, D, c)
    assert want != 0 and zk.Proof(ref.state, bad, ext_log=1, **kw).check() == want
    with pytest.raises(zk.ZkError):
        zk.Proof(ref.state, bad, ext_log=1, **kw).verify()
    with pytest.raises(zk.ZkError, match="ext_log"):
        zk.Proof(ref.state, ref.data, ext_log=2, **kw).check()
