"""Batched verification of folded proofs on the GPU (zk_verifier_set_fold, Verifier(fold_log=K)): every element of checks_out is
the number the CPU verifier zk_verify_fold gives for that proof -- for valid proofs built without the library
(tests/fold_ref.py) at every group structure, the tamper corpus (tests/verify_fold_corpus.py), a proof of the wrong factor,
batch shapes and strides, a handle that changes factor, the batch prover's own output, the benchmark domain and the C example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fold_ref
import verify_corpus
import verify_fold_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
# the four shapes of tests/test_verify_fold_corpus.py, and a 3 + 1 split on a 2-value last layer with three queries
CORPUS_SHAPES = [(5, 2, 2, 0, 2), (5, 2, 2, 8, 3), (7, 1, 1, 0, 3), (10, 3, 1, 0, 2), (4, 1, 3, 0, 3)]


def _gpu(v, items, strict, stride=None):
    plen = len(items[0].data)
    data = np.zeros((len(items), stride or plen), dtype=np.uint8)
    for r, it in enumerate(items):
        data[r, :plen] = np.frombuffer(it.data, dtype=np.uint8)
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
    return v.verify_raw(data, [it.public_last for it in items], states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n", [2, 3, 4, 5, 7, 10])
def test_valid_proofs_are_accepted(zk, orc, log_n, hash_kind):
    """Every group structure: log_n 2 with K = 3 is one short group, 3 with K = 2 is 2 + 1, 4 with K = 3 is 3 + 1, 5 with K = 3
    is 3 + 2, 7 with K = 2 is 2 + 2 + 2 + 1; log_b = 1 leaves a 2-value last layer."""
    lib = zk.load()
    for log_b in (1, 2, 3):
        for K in (2, 3):
            for q in (1, 2, 7, 64) if log_n <= 5 else (1, 2, 7):
                for g in (0, 8):
                    proofs = verify_fold_corpus.ref_proofs(orc, log_n, log_b, q, g, K, hash_kind)
                    items = [verify_corpus.Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(proofs)]
                    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K) as v:
                        assert v.proof_len == len(items[0].data)
                        for strict in (True, False):
                            cpu = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, hash_kind, strict)
                            got = _gpu(v, items, strict)
                            assert (cpu == 0).all() and (got == 0).all(), (log_b, K, q, g, strict, got, cpu)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K", CORPUS_SHAPES)
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, log_n, log_b, q, g, K, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_fold's number."""
    items = verify_fold_corpus.corpus(orc, log_n, log_b, q, g, K, hash_kind)
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K) as v:
        for strict in (True, False):
            want = verify_fold_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, g, K, hash_kind, strict)
            got = _gpu(v, items, strict)
            print(f"shape {(log_n, log_b, q, g, K)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{len(set(want.tolist()))} distinct check numbers, {(got != want).sum()} mismatches")
            assert got.shape == want.shape
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
            assert (want != 0).sum() > len(items) // 2             # the corpus is mostly rejections ...
            if not strict:
                assert len(set(want.tolist())) >= 12               # ... at many different checks


def test_a_proof_of_another_factor(zk, orc):
    """A K = 3 proof read by a K = 2 verifier, and a K = 2 proof (zero-padded) by a K = 3 verifier: rejected, with the number
    zk_verify_fold gives the first len bytes under the verifier's K."""
    log_n, log_b, q = 5, 2, 2
    proofs = {K: verify_fold_corpus.ref_proofs(orc, log_n, log_b, q, 0, K, 0) for K in (2, 3)}
    stride = max(len(proofs[2][0][0]), len(proofs[3][0][0]))
    for vk, pk in ((2, 3), (3, 2)):
        with zk.Verifier(log_n, log_b, queries=q, fold_log=vk) as v:
            plen = v.proof_len
            items = [verify_corpus.Item(f"K{pk}.p{i}", (d + bytes(stride))[:plen], s, last) for i, (d, s, last) in enumerate(proofs[pk])]
            for strict in (True, False):
                want = verify_fold_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, 0, vk, 0, strict)
                data = np.zeros((len(items), stride), dtype=np.uint8)
                for r, (d, _, _) in enumerate(proofs[pk]):
                    data[r, :len(d)] = np.frombuffer(d, dtype=np.uint8)
                states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
                got = v.verify_raw(data, [it.public_last for it in items], states)
                assert (want != 0).all() and np.array_equal(got, want), (vk, pk, strict, got, want)
            with pytest.raises(zk.ZkError):                         # Verifier.verify names the difference before any byte is read
                v.verify([zk.Proof(s, d, log_n, log_b, last, queries=q, fold_log=pk) for d, s, last in proofs[pk]])


@pytest.fixture(scope="module")
def pool(zk, orc):
    """The (5, 2, q = 2, g = 8, K = 3) SHA-256 corpus, shuffled, with the CPU's numbers, strict and plain."""
    items = verify_fold_corpus.corpus(orc, 5, 2, 2, 8, 3, 0)
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[i] for i in order]
    return items, {s: verify_fold_corpus.cpu_checks(zk.load(), items, 5, 2, 2, 8, 3, 0, s) for s in (True, False)}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
def test_batch_shapes_and_strides(zk, pool, count):
    """Counts around a wave and large; stride = len, len + 3 (unaligned rows) and len + 64, the padding noise.  Every element
    is compared: a rejection never leaks to a neighbour."""
    items, cpu = pool
    plen = len(items[0].data)
    idx = np.arange(count) % len(items)
    rng = np.random.default_rng(count)
    with zk.Verifier(5, 2, queries=2, grind_bits=8, fold_log=3) as v:
        for extra in (0, 3, 64):
            data = rng.integers(0, 256, (count, plen + extra), dtype=np.uint8)
            for r, i in enumerate(idx):
                data[r, :plen] = np.frombuffer(items[i].data, dtype=np.uint8)
            last = [items[i].public_last for i in idx]
            states = np.stack([np.frombuffer(items[i].state, dtype=np.uint8) for i in idx])
            for strict in (True, False):
                got = v.verify_raw(data, last, states if strict else None)
                assert np.array_equal(got, cpu[strict][idx]), (extra, strict)


def test_one_handle_changes_factor(zk, orc):
    """1 -> 3 -> 2 -> 1 on one handle: each run reads the format of the current factor (the buffers grow for the longer proofs),
    and back at K = 1 every result is a fresh default verifier's."""
    lib = zk.load()
    log_n, log_b = 5, 2
    k1 = verify_corpus.corpus(orc, log_n, log_b, 1, 0)
    with zk.Verifier(log_n, log_b) as fresh:
        want1 = {s: _gpu(fresh, k1, s) for s in (True, False)}
    assert len(set(want1[False].tolist())) > 10
    with zk.Verifier(log_n, log_b) as v:
        assert lib.zk_verifier_get_fold(v._h) == 1
        for K in (1, 3, 2, 1):
            v.set_fold(K)
            assert lib.zk_verifier_get_fold(v._h) == K and v.fold_log == K
            for bad in (0, 4):
                assert lib.zk_verifier_set_fold(v._h, bad) == -1 and lib.zk_verifier_get_fold(v._h) == K
                with pytest.raises(zk.ZkError):
                    v.set_fold(bad)
                assert v.fold_log == K
            for strict in (True, False):
                if K == 1:
                    assert np.array_equal(_gpu(v, k1, strict), want1[strict]), (K, strict)
                else:
                    items = verify_fold_corpus.corpus(orc, log_n, log_b, 1, 0, K, 0)
                    want = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, 1, 0, K, 0, strict)
                    got = _gpu(v, items, strict)
                    assert np.array_equal(got, want), (K, strict, _mismatches(items, got, want))


@pytest.mark.parametrize("K", [2, 3])
def test_round_trip_with_the_batch_prover(zk, K):
    """BatchContext(10, 3, 10, fold_log=K): 1 024 proofs, prove_raw()'s arrays as they are; then one flipped byte in proof 517."""
    with zk.BatchContext(10, 3, 10, fold_log=K) as bc:
        bc.gen_fibsq([1] * 1024, [3141592 + p for p in range(1024)])
        data, states = bc.prove_raw()
        last = bc.public_last()
    with zk.Verifier(10, 3, fold_log=K) as v:
        assert data.shape[1] >= v.proof_len
        assert (v.verify_raw(data, last, states) == 0).all()
        assert (v.verify_raw(data, last) == 0).all()
        data[517, 3000] ^= 0x20
        for strict in (True, False):
            got = v.verify_raw(data, last, states if strict else None)
            want = zk.Proof(states[517].tobytes(), data[517, :v.proof_len].tobytes(), 10, 3, int(last[517]), fold_log=K).check(strict)
            assert want != 0 and got[517] == want
            assert (np.delete(got, 517) == 0).all()


@pytest.mark.parametrize("q", [1, 16])
def test_benchmark_domain_2e24(zk, q):
    """Two 2^24 proofs (log_n 21) folded by 8, strict: accepted; a tampered node of a path of the last group (G = 7: j = 6) gives
    the CPU's -306 for t = 0 and -406 for t >= 1."""
    log_n, log_b, K = 21, 3, 3
    with zk.BatchContext(log_n, log_b, 1, queries=q, fold_log=K) as bc:
        bc.gen_fibsq([1, 1], [3141592, 3141593])
        data, states = bc.prove_raw()
        last = bc.public_last()
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K) as v:
        plen = v.proof_len
        assert (v.verify_raw(data, last, states) == 0).all()
        fields = {name: off for name, off, _, _ in verify_fold_corpus.fields(log_n, log_b, q, 0, K)}
        for t, want_check in ((0, -306), (5, -406)):
            bad = data.copy()
            off = [o for n, o in fields.items() if n.startswith(f"q0.group6.p{t}.node")][0]
            bad[1, off + 7] ^= 0x04
            for strict in (True, False):
                got = v.verify_raw(bad, last, states if strict else None)
                cpu = zk.Proof(states[1].tobytes(), bad[1, :plen].tobytes(), log_n, log_b, int(last[1]), queries=q, fold_log=K).check(strict)
                assert got[0] == 0 and got[1] == cpu
                assert cpu == (-1999 if strict else want_check)


def test_verify_c_abi_folded_from_plain_c(tmp_path):
    """examples/verify_c_abi.c with fold_log 3: 64 folded proofs from zk_batch_prove, one corrupted, one zk_verifier_run."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "verify_c_abi")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "verify_c_abi.c"),
                           "-L" + os.path.join(root, "zkstark_amd"), "-lzkstark_amd",
                           "-Wl,-rpath," + os.path.join(root, "zkstark_amd"), "-o", exe])
    out = subprocess.run([exe, "17", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "strict: 63 of 64 proofs accepted" in out.stdout and "plain: 63 of 64 proofs accepted" in out.stdout
    assert "strict: proof 17 rejected at check -1999" in out.stdout
    gpu = re.search(r"^plain: proof 17 rejected at check (-\d+)$", out.stdout, re.M)
    cpu = re.search(r"^cpu plain: proof 17 check (-\d+)$", out.stdout, re.M)
    assert gpu and cpu and gpu.group(1) == cpu.group(1) == "-4", out.stdout
