"""Batched verification of proofs with coset leaves on the GPU (zk_verifier_set_coset_leaves, Verifier(coset_leaves=True)): every
element of checks_out is the number the CPU verifier zk_verify_coset gives for that proof -- for valid proofs built without the
library (tests/coset_ref.py) at every group structure and K = 1, 2, 3, the tamper corpus (tests/verify_coset_corpus.py), proofs of
another format, batch shapes and strides, and a handle that changes format between runs."""
import numpy as np
import pytest

import verify_corpus
import verify_coset_corpus
import verify_fold_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
# the shapes of tests/test_verify_coset_corpus.py: 2+2+1, 3+2 with a nonce and seven queries (every rotation of an 8-slot leaf),
# 3+3+1 on a 2-value last layer, K = 1 at the reference's size, 3+1 with three queries
CORPUS_SHAPES = [(5, 2, 2, 0, 2), (5, 2, 7, 8, 3), (7, 1, 1, 0, 3), (10, 3, 1, 0, 1), (4, 1, 3, 0, 3)]


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
    """Every group structure: K = 1 is log_n groups of two slots; log_n 2 with K = 3 is one short group, 3 with K = 2 is 2 + 1, 4
    with K = 3 is 3 + 1, 5 with K = 3 is 3 + 2, 7 with K = 2 is 2 + 2 + 2 + 1; log_b = 1 leaves a 2-value last layer and group
    paths of one digest."""
    lib = zk.load()
    for log_b in (1, 2, 3):
        for K in (1, 2, 3):
            for q in (1, 2, 7, 64) if log_n <= 5 else (1, 2, 7):
                for g in (0, 8):
                    proofs = verify_coset_corpus.ref_proofs(orc, log_n, log_b, q, g, K, hash_kind)
                    items = [verify_corpus.Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(proofs)]
                    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=True) as v:
                        assert v.proof_len == len(items[0].data)
                        for strict in (True, False):
                            cpu = verify_coset_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, hash_kind, strict)
                            got = _gpu(v, items, strict)
                            assert (cpu == 0).all() and (got == 0).all(), (log_b, K, q, g, strict, got, cpu)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K", CORPUS_SHAPES)
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, log_n, log_b, q, g, K, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_coset's number."""
    items = verify_coset_corpus.corpus(orc, log_n, log_b, q, g, K, hash_kind)
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=True) as v:
        for strict in (True, False):
            want = verify_coset_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, g, K, hash_kind, strict)
            got = _gpu(v, items, strict)
            print(f"shape {(log_n, log_b, q, g, K)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{len(set(want.tolist()))} distinct check numbers, {(got != want).sum()} mismatches")
            assert got.shape == want.shape
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
            assert (want != 0).sum() > len(items) // 2             # the corpus is mostly rejections


def _padded(proofs, plen, tag):
    """The proofs cut or zero-padded to plen bytes, as Items."""
    return [verify_corpus.Item(f"{tag}.p{i}", (d + bytes(plen))[:plen], s, last) for i, (d, s, last) in enumerate(proofs)]


@pytest.mark.parametrize("case", ["plain_by_coset", "coset_by_plain", "coset_k3_by_coset_k2"])
def test_a_proof_of_another_format(zk, orc, case):
    """(5, 2, q = 2): a plain K = 2 proof read by a coset K = 2 verifier, a coset K = 2 proof by a plain K = 2 verifier, a coset
    K = 3 proof by a coset K = 2 verifier.  Each is rejected with the number the CPU verifier of the verifier's settings gives the
    first proof_len bytes, and Verifier.verify names the difference before any byte is read."""
    log_n, log_b, q = 5, 2, 2
    plain2 = verify_fold_corpus.ref_proofs(orc, log_n, log_b, q, 0, 2, 0)
    coset = {K: verify_coset_corpus.ref_proofs(orc, log_n, log_b, q, 0, K, 0) for K in (2, 3)}
    proofs, p_coset, p_fold, v_coset = {"plain_by_coset": (plain2, False, 2, True), "coset_by_plain": (coset[2], True, 2, False),
                                        "coset_k3_by_coset_k2": (coset[3], True, 3, True)}[case]
    with zk.Verifier(log_n, log_b, queries=q, fold_log=2, coset_leaves=v_coset) as v:
        plen = v.proof_len
        assert plen != len(proofs[0][0])
        items = _padded(proofs, plen, case)
        stride = max(plen, len(proofs[0][0]))
        for strict in (True, False):
            want = verify_coset_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, 0, 2, 0, strict,
                                                  fn="zk_verify_coset" if v_coset else "zk_verify_fold")
            data = np.zeros((len(items), stride), dtype=np.uint8)
            for r, (d, _, _) in enumerate(proofs):
                data[r, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
            got = v.verify_raw(data, [it.public_last for it in items], states)
            assert (want != 0).all() and np.array_equal(got, want), (case, strict, got, want)
        with pytest.raises(zk.ZkError) as err:
            v.verify([zk.Proof(s, d, log_n, log_b, last, queries=q, fold_log=p_fold, coset_leaves=p_coset) for d, s, last in proofs])
        assert ("leaves" in str(err.value)) if p_coset != v_coset else ("fold_log" in str(err.value))


@pytest.fixture(scope="module")
def pool(zk, orc):
    """The (5, 2, q = 7, g = 8, K = 3) SHA-256 corpus, shuffled, with the CPU's numbers, strict and plain."""
    items = verify_coset_corpus.corpus(orc, 5, 2, 7, 8, 3, 0)
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[i] for i in order]
    return items, {s: verify_coset_corpus.cpu_checks(zk.load(), items, 5, 2, 7, 8, 3, 0, s) for s in (True, False)}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
def test_batch_shapes_and_strides(zk, pool, count):
    """Counts around a wave and large; stride = len, len + 3 (unaligned rows) and len + 64, the padding noise.  Every element
    is compared: a rejection never leaks to a neighbour."""
    items, cpu = pool
    plen = len(items[0].data)
    idx = np.arange(count) % len(items)
    rng = np.random.default_rng(count)
    with zk.Verifier(5, 2, queries=7, grind_bits=8, fold_log=3, coset_leaves=True) as v:
        for extra in (0, 3, 64):
            data = rng.integers(0, 256, (count, plen + extra), dtype=np.uint8)
            for r, i in enumerate(idx):
                data[r, :plen] = np.frombuffer(items[i].data, dtype=np.uint8)
            last = [items[i].public_last for i in idx]
            states = np.stack([np.frombuffer(items[i].state, dtype=np.uint8) for i in idx])
            for strict in (True, False):
                got = v.verify_raw(data, last, states if strict else None)
                assert np.array_equal(got, cpu[strict][idx]), (extra, strict)


def test_one_handle_changes_format(zk, orc):
    """(off, K 1) -> (on, K 3) -> (on, K 1) -> (off, K 2) -> (off, K 1) on one handle: each run reads the format of the current
    settings, the getter tracks every change, and back at the defaults every result is a fresh default verifier's."""
    lib = zk.load()
    log_n, log_b = 5, 2
    k1 = verify_corpus.corpus(orc, log_n, log_b, 1, 0)
    with zk.Verifier(log_n, log_b) as fresh:
        want1 = {s: _gpu(fresh, k1, s) for s in (True, False)}
    assert len(set(want1[False].tolist())) > 10
    with zk.Verifier(log_n, log_b) as v:
        assert lib.zk_verifier_get_coset_leaves(v._h) == 0 and v.coset_leaves is False
        for step, (on, K) in enumerate(((False, 1), (True, 3), (True, 1), (False, 2), (False, 1))):
            v.set_fold(K)
            if step == 1:
                assert lib.zk_verifier_set_coset_leaves(v._h, 7) == 0        # any non-zero value means on
                v.coset_leaves = True
            else:
                v.set_coset_leaves(on)
            assert lib.zk_verifier_get_coset_leaves(v._h) == int(on) and v.coset_leaves == on
            assert lib.zk_verifier_get_fold(v._h) == K and v.fold_log == K
            assert v.proof_len == (lib.zk_proof_data_len_coset if on else lib.zk_proof_data_len_fold)(log_n, log_b, 1, 0, K)
            for strict in (True, False):
                if on:
                    items = verify_coset_corpus.corpus(orc, log_n, log_b, 1, 0, K, 0)
                    want = verify_coset_corpus.cpu_checks(lib, items, log_n, log_b, 1, 0, K, 0, strict)
                elif K != 1:
                    items = verify_fold_corpus.corpus(orc, log_n, log_b, 1, 0, K, 0)
                    want = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, 1, 0, K, 0, strict)
                else:
                    items = k1
                    want = verify_fold_corpus.cpu_checks(lib, items, log_n, log_b, 1, 0, 1, 0, strict)
                    if step == 4:
                        assert np.array_equal(want, want1[strict])
                got = _gpu(v, items, strict)
                assert np.array_equal(got, want), (on, K, strict, _mismatches(items, got, want))
