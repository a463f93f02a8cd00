"""Batched verification of proofs that stop FRI early on the GPU (zk_verifier_set_fri_stop, Verifier(stop_log=D)): every element
of checks_out is the number the CPU verifier zk_verify_stop gives for that proof -- for valid proofs built without the library
(tests/stop_ref.py) at every group structure, K = 1, 2, 3 and both leaf formats, the tamper corpus (tests/verify_stop_corpus.py),
proofs of another format, batch shapes and strides, and a handle that changes format between runs.  No proof here comes from the
library's prover."""
import numpy as np
import pytest

import stop_ref
import verify_corpus
import verify_fold_corpus
import verify_stop_corpus

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
CORPUS_SHAPES = verify_stop_corpus.SHAPES
LOG_NS = [2, 3, 4, 5, 7, 10]
QG = [(1, 0), (2, 8), (7, 0), (1, 8), (2, 0), (7, 8)]        # every q in 1, 2, 7 with g = 0 and with g = 8


def _structures(log_n):
    """(log_b, K, coset, D, q, g) of the valid-proof test: every K, leaf format and admissible D of {1, 2, log_n - 1, 8}, with every
    log_b of 1, 2, 3 up to log_n = 5; the proofs come from Python (tests/stop_ref.py), so at log_n = 7 and 10 the three log_b are
    taken in turn instead (log_b = 1 for the 256-coefficient interpolation at log_n = 10), and so are the (q, g) pairs everywhere."""
    out = []
    for K in (1, 2, 3):
        for coset in (False, True):
            for D in sorted({1, 2, log_n - 1, 8}):
                for log_b in (1, 2, 3) if log_n <= 5 else (1 if D == 8 else 1 + len(out) % 3,):
                    if stop_ref.admissible(log_n, log_b, D):
                        out.append((log_b, K, coset, D) + QG[len(out) % len(QG)])
    return out


def test_structures_keep_every_last_group():
    """The trimmed product still has every (K, leaf format, steps of the last group), every q and g, and D = 8."""
    seen, qs, ds, lbs = set(), set(), set(), set()
    for log_n in LOG_NS:
        for log_b, K, coset, D, q, g in _structures(log_n):
            grp = stop_ref.groups(log_n - D, K)
            seen.add((K, coset, grp[-1][1]))
            qs.add((q, g))
            ds.add(D)
            if log_n >= 7:
                lbs.add(log_b)
    assert seen == {(K, c, ls) for K in (1, 2, 3) for c in (False, True) for ls in range(1, K + 1)}
    assert qs == set(QG) and {1, 2, 8} <= ds and lbs == {1, 2, 3}


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
@pytest.mark.parametrize("log_n", LOG_NS)
def test_valid_proofs_are_accepted(zk, orc, log_n, hash_kind):
    """Every structure of the folded rounds R' = log_n - D: one short group, full groups only, a short last group of one or two
    steps, R' = 1 with no group root in the header at all."""
    lib = zk.load()
    for log_b, K, coset, D, q, g in _structures(log_n):
        proofs = verify_stop_corpus.ref_proofs(orc, log_n, log_b, q, g, K, coset, D, hash_kind)
        items = [verify_corpus.Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(proofs)]
        with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D) as v:
            assert v.proof_len == len(items[0].data)
            assert lib.zk_verifier_get_fri_stop(v._h) == D and v.stop_log == D
            for strict in (True, False):
                cpu = verify_stop_corpus.cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, hash_kind, strict)
                got = _gpu(v, items, strict)
                assert (cpu == 0).all() and (got == 0).all(), (log_b, K, coset, D, q, g, strict, got, cpu)


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_n,log_b,q,g,K,coset,D", CORPUS_SHAPES)
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, log_n, log_b, q, g, K, coset, D, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_stop's number."""
    items = verify_stop_corpus.corpus(orc, log_n, log_b, q, g, K, coset, D, hash_kind)
    with zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D) as v:
        for strict in (True, False):
            want = verify_stop_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, g, K, coset, D, hash_kind, strict)
            got = _gpu(v, items, strict)
            print(f"shape {(log_n, log_b, q, g, K, coset, D)} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{len(set(want.tolist()))} distinct check numbers, {(got != want).sum()} mismatches")
            assert got.shape == want.shape
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
            assert (want != 0).sum() > len(items) // 2             # the corpus is mostly rejections


@pytest.mark.parametrize("case", ["d2_by_d0", "d0_by_d2", "d2_by_d4"])
def test_a_proof_of_another_format(zk, orc, case):
    """(5, 2, q = 2, K = 2, one-value leaves): a D = 2 proof read by a D = 0 verifier, a D = 0 proof by a D = 2 verifier, a D = 2
    proof by a D = 4 verifier, each cut or zero-padded to the verifier's length.  Each is rejected with the number zk_verify_stop of
    the verifier's settings gives those bytes, and Verifier.verify names the difference before any byte is read."""
    log_n, log_b, q, K = 5, 2, 2, 2
    p_d, v_d = {"d2_by_d0": (2, 0), "d0_by_d2": (0, 2), "d2_by_d4": (2, 4)}[case]
    proofs = verify_stop_corpus.ref_proofs(orc, log_n, log_b, q, 0, K, False, p_d, 0) if p_d else verify_fold_corpus.ref_proofs(orc, log_n, log_b, q, 0, K, 0)
    with zk.Verifier(log_n, log_b, queries=q, fold_log=K, stop_log=v_d) as v:
        plen = v.proof_len
        assert plen != len(proofs[0][0])
        items = [verify_corpus.Item(f"{case}.p{i}", (d + bytes(plen))[:plen], s, last) for i, (d, s, last) in enumerate(proofs)]
        stride = max(plen, len(proofs[0][0]))
        for strict in (True, False):
            want = verify_stop_corpus.cpu_checks(zk.load(), items, log_n, log_b, q, 0, K, False, v_d, 0, strict)
            data = np.zeros((len(items), stride), dtype=np.uint8)
            for r, (d, _, _) in enumerate(proofs):
                data[r, :len(d)] = np.frombuffer(d, dtype=np.uint8)
            states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
            got = v.verify_raw(data, [it.public_last for it in items], states)
            assert (want != 0).all() and np.array_equal(got, want), (case, strict, got, want)
        with pytest.raises(zk.ZkError) as err:
            v.verify([zk.Proof(s, d, log_n, log_b, last, queries=q, fold_log=K, stop_log=p_d) for d, s, last in proofs])
        assert "stop_log" in str(err.value)


POOL = (5, 2, 7, 8, 3, True, 2)


@pytest.fixture(scope="module")
def pool(zk, orc):
    """The (5, 2, q = 7, g = 8, K = 3, coset leaves, D = 2) SHA-256 corpus, shuffled, with the CPU's numbers, strict and plain."""
    items = verify_stop_corpus.corpus(orc, *POOL, 0)
    order = np.random.default_rng(7).permutation(len(items))
    items = [items[i] for i in order]
    return items, {s: verify_stop_corpus.cpu_checks(zk.load(), items, *POOL, 0, s) for s in (True, False)}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
def test_batch_shapes_and_strides(zk, pool, count):
    """Counts around a wave and large; stride = len, len + 3 (unaligned rows) and len + 64, the padding noise.  Every element
    is compared: a rejection never leaks to a neighbour."""
    items, cpu = pool
    plen = len(items[0].data)
    idx = np.arange(count) % len(items)
    rng = np.random.default_rng(count)
    log_n, log_b, q, g, K, coset, D = POOL
    with zk.Verifier(log_n, log_b, queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D) as v:
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
    """(D 0, K 1, off) -> (D 2, K 3, on) -> (D 1, K 1, off) -> (D 0, K 2, off) -> (D 0, K 1, off) on one handle: each run reads the
    format of the current settings, the getter tracks every change, and back at the defaults every result is a fresh default
    verifier's.  A value outside the limits is refused and leaves the setting as it was."""
    lib = zk.load()
    log_n, log_b = 5, 2
    k1 = verify_corpus.corpus(orc, log_n, log_b, 1, 0)
    with zk.Verifier(log_n, log_b) as fresh:
        want1 = {s: _gpu(fresh, k1, s) for s in (True, False)}
    assert len(set(want1[False].tolist())) > 10
    assert lib.zk_verifier_get_fri_stop(None) == 0 and lib.zk_verifier_set_fri_stop(None, 1) == -1     # ZK_ERR_INVALID
    with zk.Verifier(log_n, log_b) as v:
        assert lib.zk_verifier_get_fri_stop(v._h) == 0 and v.stop_log == 0
        for step, (D, K, on) in enumerate(((0, 1, False), (2, 3, True), (1, 1, False), (0, 2, False), (0, 1, False))):
            if step % 2:                                      # no order between the setters
                v.set_fri_stop(D); v.set_fold(K); v.set_coset_leaves(on)
            else:
                v.set_coset_leaves(on); v.set_fold(K); v.set_fri_stop(D)
            for bad in (5, 9):                                # (5, 2): D <= log_n - 1 = 4 and D <= 8
                assert lib.zk_verifier_set_fri_stop(v._h, bad) == -1
                with pytest.raises(zk.ZkError):
                    v.set_fri_stop(bad)
            assert lib.zk_verifier_get_fri_stop(v._h) == D and v.stop_log == D
            assert lib.zk_verifier_get_fold(v._h) == K and lib.zk_verifier_get_coset_leaves(v._h) == int(on)
            assert v.proof_len == lib.zk_proof_data_len_stop(log_n, log_b, 1, 0, K, int(on), D)
            for strict in (True, False):
                if D:
                    items = verify_stop_corpus.corpus(orc, log_n, log_b, 1, 0, K, on, D, 0)
                elif K != 1:
                    items = verify_fold_corpus.corpus(orc, log_n, log_b, 1, 0, K, 0)
                else:
                    items = k1
                want = verify_stop_corpus.cpu_checks(lib, items, log_n, log_b, 1, 0, K, on, D, 0, strict)
                if step == 4:
                    assert np.array_equal(want, want1[strict])
                got = _gpu(v, items, strict)
                assert np.array_equal(got, want), (D, K, on, strict, _mismatches(items, got, want))
    with zk.Verifier(10, 5) as v:                             # D + log_blowup <= 12
        assert lib.zk_verifier_set_fri_stop(v._h, 8) == -1 and lib.zk_verifier_get_fri_stop(v._h) == 0
        assert lib.zk_verifier_set_fri_stop(v._h, 7) == 0 and lib.zk_verifier_get_fri_stop(v._h) == 7
        assert lib.zk_verifier_set_fri_stop(v._h, 8) == -1 and lib.zk_verifier_get_fri_stop(v._h) == 7
