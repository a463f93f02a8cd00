"""Batched verification on the GPU (zk_verifier_*, Verifier): every element of checks_out is the number the CPU verifier
(zk_verify_check, Proof.check) gives for that proof -- accepted, rejected, and at which check -- for valid proofs, the
whole tamper corpus (tests/verify_corpus.py), batch shapes and strides, the batch prover's own output and the benchmark domain."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import verify_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}


def _cpu(zk, items, log_n, log_b, q, hash_kind, strict):
    return np.array([zk.Proof(it.state, it.data, log_n, log_b, it.public_last, HASH_NAMES[hash_kind], q).check(strict) for it in items],
                    dtype=np.int32)


def _gpu(zk, items, log_n, log_b, q, hash_kind, strict):
    data = np.stack([np.frombuffer(it.data, dtype=np.uint8) for it in items])
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q) as v:
        return v.verify_raw(data, [it.public_last for it in items], states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n", [2, 4, 5, 10, 13])
def test_valid_proofs_are_accepted(zk, orc, log_n, hash_kind):
    for log_b in (1, 2, 3):
        for q in (1, 2, 7, 64):
            proofs = verify_corpus.oracle_proofs(orc, log_n, log_b, q, hash_kind)
            items = [verify_corpus.Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(proofs)]
            for strict in (True, False):
                cpu = _cpu(zk, items, log_n, log_b, q, hash_kind, strict)
                got = _gpu(zk, items, log_n, log_b, q, hash_kind, strict)
                assert (cpu == 0).all() and (got == 0).all(), (log_b, q, strict, got, cpu)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q", [(10, 3, 1), (5, 2, 1), (5, 2, 3)])
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, log_n, log_b, q, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_check's number."""
    items = verify_corpus.corpus(orc, log_n, log_b, q, hash_kind)
    for strict in (True, False):
        want = _cpu(zk, items, log_n, log_b, q, hash_kind, strict)
        got = _gpu(zk, items, log_n, log_b, q, hash_kind, strict)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
        assert (want != 0).sum() > len(items) // 2             # the corpus is mostly rejections, at many different checks
        assert len(set(want.tolist())) > 10


@pytest.fixture(scope="module")
def pool(zk, orc):
    """The (5, 2) SHA-256 corpus: valid and tampered proofs interleaved, with the CPU's numbers, strict and plain."""
    items = verify_corpus.corpus(orc, 5, 2, 1, 0)
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[i] for i in order]
    return items, {s: _cpu(zk, items, 5, 2, 1, 0, s) for s in (True, False)}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000, 4096])
def test_batch_shapes_and_strides(zk, pool, count):
    """Counts around a wave and large; stride = len, len + 3 (unaligned rows) and len + 64.  A rejection never leaks to a
    neighbour: every element is compared."""
    items, cpu = pool
    plen = len(items[0].data)
    idx = np.arange(count) % len(items)
    rng = np.random.default_rng(count)
    with zk.Verifier(5, 2) as v:
        for extra in (0, 3, 64):
            data = rng.integers(0, 256, (count, plen + extra), dtype=np.uint8)      # the padding is noise
            for r, i in enumerate(idx):
                data[r, :plen] = np.frombuffer(items[i].data, dtype=np.uint8)
            last = [items[i].public_last for i in idx]
            states = np.stack([np.frombuffer(items[i].state, dtype=np.uint8) for i in idx])
            for strict in (True, False):
                got = v.verify_raw(data, last, states if strict else None)
                assert np.array_equal(got, cpu[strict][idx]), (extra, strict)


def test_round_trip_with_the_batch_prover(zk):
    """BatchContext(10, 3, 10): 1 024 proofs, prove_raw()'s arrays as they are; then one flipped byte in proof 517."""
    with zk.BatchContext(10, 3, 10) as bc:
        bc.gen_fibsq([1] * 1024, [3141592 + p for p in range(1024)])
        data, states = bc.prove_raw()
        last = bc.public_last()
    with zk.Verifier(10, 3) as v:
        assert (v.verify_raw(data, last, states) == 0).all()
        assert (v.verify_raw(data, last) == 0).all()
        data[517, 3000] ^= 0x20
        for strict in (True, False):
            got = v.verify_raw(data, last, states if strict else None)
            want = zk.Proof(states[517].tobytes(), data[517].tobytes(), 10, 3, int(last[517])).check(strict)
            assert want != 0 and got[517] == want
            assert (np.delete(got, 517) == 0).all()


@pytest.mark.parametrize("q", [1, 16])
def test_benchmark_domain_2e24(zk, q):
    """Two 2^24 proofs (log_n 21), strict: accepted; a tampered node of a layer-20 path gives the CPU's -(300+20) / -(400+20)."""
    log_n, log_b = 21, 3
    with zk.BatchContext(log_n, log_b, 1, queries=q) as bc:
        bc.gen_fibsq([1, 1], [3141592, 3141593])
        data, states = bc.prove_raw()
        last = bc.public_last()
    with zk.Verifier(log_n, log_b, queries=q) as v:
        assert (v.verify_raw(data, last, states) == 0).all()
        fields = {name: (off, size) for name, off, size, _ in verify_corpus.fields(log_n, log_b, q)}
        for which, want_check in (("x", -320), ("nx", -420)):
            bad = data.copy()
            name = [n for n in fields if n.startswith(f"q0.layer20.{which}_node")][0]
            off, _ = fields[name]
            bad[1, off + 7] ^= 0x04
            for strict in (True, False):
                got = v.verify_raw(bad, last, states if strict else None)
                cpu = zk.Proof(states[1].tobytes(), bad[1].tobytes(), log_n, log_b, int(last[1]), queries=q).check(strict)
                assert got[0] == 0 and got[1] == cpu
                assert cpu == (-1999 if strict else want_check)


def test_argument_errors(zk, orc):
    from zkstark_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for log_n, log_b in ((1, 3), (10, 0), (25, 6)):
        assert lib.zk_verifier_create(0, log_n, log_b, C.byref(h)) == -1 and not h.value
    assert lib.zk_verifier_create(0, 5, 2, None) == -1
    (d0, s0, l0), (d1, s1, l1) = verify_corpus.oracle_proofs(orc, 5, 2, 1, 0)
    plen = len(d0)
    data = np.frombuffer(d0 + d1, dtype=np.uint8).copy()
    states = np.frombuffer(s0 + s1, dtype=np.uint8).copy()
    last = np.array([l0, l1], dtype=np.uint32)
    out = np.full(2, 99, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                                   # noqa: E731
    assert lib.zk_verifier_create(0, 5, 2, C.byref(h)) == 0 and h.value
    try:
        assert lib.zk_verifier_set_hash(h, 2) == -1 and lib.zk_verifier_set_hash(h, -1) == -1
        assert lib.zk_verifier_set_queries(h, 0) == -1 and lib.zk_verifier_set_queries(h, 65) == -1
        assert lib.zk_verifier_run(h, ptr(data), plen - 1, 2, ptr(states), ptr(last), ptr(out)) == -1
        assert lib.zk_verifier_run(h, None, plen, 2, ptr(states), ptr(last), ptr(out)) == -1
        assert lib.zk_verifier_run(h, ptr(data), plen, 2, ptr(states), None, ptr(out)) == -1
        assert lib.zk_verifier_run(None, ptr(data), plen, 2, ptr(states), ptr(last), ptr(out)) == -1
        assert (out == 99).all()                                                   # nothing written
        assert lib.zk_verifier_run(h, None, plen, 0, None, None, None) == 0        # count = 0 is a no-op
        assert lib.zk_verifier_run(h, ptr(data), plen, 2, ptr(states), ptr(last), ptr(out)) == 0 and (out == 0).all()
        assert lib.zk_verifier_set_hash(h, 0) == 0 and lib.zk_verifier_set_queries(h, 64) == 0
        big = np.zeros(2 * plen, dtype=np.uint8)                                   # stride too small for 64 queries
        assert lib.zk_verifier_run(h, ptr(big), plen, 2, None, ptr(last), ptr(out)) == -1
    finally:
        lib.zk_verifier_destroy(h)
    with pytest.raises(zk.ZkError):
        zk.Verifier(5, 2, hash="md5")


def test_verify_c_abi_from_plain_c(tmp_path):
    """examples/verify_c_abi.c: 64 proofs from zk_batch_prove, one corrupted, all verified with one zk_verifier_run from C."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "verify_c_abi")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "verify_c_abi.c"),
                           "-L" + os.path.join(root, "zkstark_amd"), "-lzkstark_amd",
                           "-Wl,-rpath," + os.path.join(root, "zkstark_amd"), "-o", exe])
    out = subprocess.run([exe, "17"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "strict: proof 17 rejected at check -1999" in out.stdout       # the path bytes are part of the transcript
    assert "plain: proof 17 rejected at check -4" in out.stdout           # the f(x) path (proof.rs:80-95)
    assert "cpu plain: proof 17 check -4" in out.stdout
    assert "strict: 63 of 64 proofs accepted" in out.stdout and "plain: 63 of 64 proofs accepted" in out.stdout
