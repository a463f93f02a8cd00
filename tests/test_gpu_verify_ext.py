"""Batched verification of proofs over E = F_P[u] / (u^2 - 5) on the GPU (zk_verifier_set_ext, Verifier(ext_log=1)): every
element of checks_out is the number the CPU verifier zk_verify_ext gives for that proof -- for valid proofs built without the library
(tests/ext_ref.py) over the grid of settings, the tamper corpus (tests/verify_ext_corpus.py), two broken fields whose wire order decides
the number, batch shapes and strides, proofs of the other format, one handle walked between ext off and on, the one-call prover's own
proofs, and the refusals on a live handle.  The expected value is never the GPU's own output."""
import numpy as np
import pytest

import ext_ref
import verify_cap_corpus
import verify_ext_corpus
from verify_corpus import Item

gpu = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}

# (log_n, log_b, q, hash, K, coset, D, cap, grinding bits): every K x leaf format, D in {0, 2}, cap in {0, 4, 8}, q in {1, 16}, grinding in
# {0, 8}, both hashes and the three sizes occur (test_the_grid_covers_every_value); D = 2 needs log_n >= 3.  Thinned as the grid of
# tests/test_ext_verify.py is: the proofs come from Python, so q = 16 stays at the two small sizes.
SETTINGS = [
    (2, 1, 1, 0, 1, False, 0, 0, 0),
    (2, 1, 16, 1, 2, True, 0, 4, 8),
    (4, 2, 1, 0, 1, True, 0, 4, 0),
    (4, 2, 16, 1, 1, False, 2, 0, 8),
    (4, 2, 1, 1, 2, False, 0, 8, 0),
    (4, 2, 16, 0, 2, True, 2, 4, 0),
    (4, 2, 1, 0, 3, False, 2, 4, 8),
    (4, 2, 16, 0, 3, True, 0, 8, 0),
    (4, 2, 1, 1, 3, True, 0, 0, 0),
    (10, 3, 1, 0, 1, False, 0, 4, 0),
    (10, 3, 1, 1, 1, True, 2, 0, 0),
    (10, 3, 1, 0, 2, False, 2, 8, 8),
    (10, 3, 1, 1, 2, True, 0, 0, 0),
    (10, 3, 1, 1, 3, False, 0, 8, 0),
    (10, 3, 1, 0, 3, True, 2, 4, 8),
]


def test_the_grid_covers_every_value():
    assert {(s[4], s[5]) for s in SETTINGS} == {(k, c) for k in (1, 2, 3) for c in (False, True)}
    assert {s[6] for s in SETTINGS} == {0, 2} and {s[7] for s in SETTINGS} == {0, 4, 8}
    assert {s[2] for s in SETTINGS} == {1, 16} and {s[8] for s in SETTINGS} == {0, 8} and {s[3] for s in SETTINGS} == {0, 1}
    assert {s[:2] for s in SETTINGS} == {(2, 1), (4, 2), (10, 3)}
    # the 16-word leaf of a full K = 3 group with coset leaves, under both hashes
    assert {s[3] for s in SETTINGS if s[4] == 3 and s[5] and s[0] - s[6] >= 3} == {0, 1}


def _gpu(v, items, strict, stride=None):
    plen = len(items[0].data)
    data = np.zeros((len(items), stride or plen), dtype=np.uint8)
    for r, it in enumerate(items):
        data[r, :plen] = np.frombuffer(it.data, dtype=np.uint8)
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
    return v.verify_raw(data, [it.public_last for it in items], states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


def _verifier(zk, log_n, log_b, q, g, K, coset, D, c, hash_kind=0, ext_log=1):
    return zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c,
                       ext_log=ext_log)


# ---- 1. valid proofs ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_valid_proofs_are_accepted(zk, orc, setting):
    log_n, log_b, q, hash_kind, K, coset, D, c, bits = setting
    lib = zk.load()
    refs = [ext_ref.proof(orc, log_n, log_b, q, hash_kind, K, coset, D, c, bits, a1) for a1 in verify_ext_corpus.SEEDS]
    items = [Item(f"p{i}", r.data, r.state, r.public_last) for i, r in enumerate(refs)]
    with _verifier(zk, log_n, log_b, q, bits, K, coset, D, c, hash_kind) as v:
        assert v.proof_len == len(items[0].data) == lib.zk_proof_data_len_ext(log_n, log_b, q, bits, K, int(coset), D, c, 1)
        assert lib.zk_verifier_get_ext(v._h) == 1 and v.ext_log == 1
        for strict in (True, False):
            cpu = verify_ext_corpus.cpu_checks(lib, items, log_n, log_b, q, bits, K, coset, D, c, hash_kind, strict)
            got = _gpu(v, items, strict)
            assert (cpu == 0).all() and (got == 0).all(), (setting, strict, got, cpu)


# ---- 2. the tamper corpus ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", verify_ext_corpus.SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, shape, hash_kind):
    """The exactness claim: for every element of the corpus, strict and plain, checks_out[i] == zk_verify_ext's number."""
    items = verify_ext_corpus.corpus(orc, *shape, hash_kind)
    with _verifier(zk, *shape, hash_kind) as v:
        for strict in (True, False):
            want = verify_ext_corpus.cpu_checks(zk.load(), items, *shape, hash_kind, strict)
            got = _gpu(v, items, strict)
            print(f"shape {shape} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{len(set(want.tolist()))} distinct check numbers, {(got != want).sum()} mismatches")
            assert got.shape == want.shape
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
            assert (want != 0).sum() > len(items) // 2             # the corpus is mostly rejections


# ---- 3. two broken fields whose wire order decides the number ------------------------------------------------------------------------
def _region(shape, name):
    for n, off, size in ext_ref.regions(*shape):
        if n == name:
            return off, size
    raise KeyError(name)


def _broken(data, shape, names):
    bad = bytearray(data)
    for name in names:
        off, size = _region(shape, name)
        bad[off + size - 1] ^= 0x40                              # the last byte: of a path its last node
    return bytes(bad)


ORDER_CASES = [
    # a later query's f path against an earlier query's group path: verify_proof_ext meets query 0's group first
    ("f_path_q1_vs_group_path_q0.values", (6, 1, 2, 0, 3, False, 0, 8), ("q1.f0.path", "q0.g1.path5"), -401),
    ("f_path_q1_vs_group_path_q0.coset", (4, 2, 2, 8, 3, True, 0, 0), ("q1.f0.path", "q0.g1.path0"), -301),
    # a fold that fails only in component 1 (the free term's, or a coefficient's, c1 word) against a path of the same query: every fold of a
    # query comes before its group paths
    ("fold_c1_vs_group_path.values", (6, 1, 2, 0, 3, False, 0, 8), ("free_term.c1", "q0.g0.path3"), -101),
    ("fold_c1_vs_group_path.coset", (7, 2, 3, 8, 2, True, 4, 4), ("coef5.c1", "q0.g0.path0"), -101),
]


@gpu
@pytest.mark.parametrize("label,shape,names,number", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_the_first_failure_in_wire_order_wins(zk, orc, label, shape, names, number):
    lib = zk.load()
    for hash_kind in (0, 1):
        refs = verify_ext_corpus.ref_objects(orc, *shape, hash_kind)
        items = [Item("valid", refs[1].data, refs[1].state, refs[1].public_last)]
        items += [Item(f"{label}.{n}", _broken(refs[0].data, shape, [n]), refs[0].state, refs[0].public_last) for n in names]
        items.append(Item(label, _broken(refs[0].data, shape, names), refs[0].state, refs[0].public_last))
        with _verifier(zk, *shape, hash_kind) as v:
            for strict in (True, False):
                want = verify_ext_corpus.cpu_checks(lib, items, *shape, hash_kind, strict)
                got = _gpu(v, items, strict)
                assert np.array_equal(got, want), (label, hash_kind, strict, _mismatches(items, got, want))
                if not strict:
                    assert want[0] == 0 and want[1] != want[2] and want[1] != 0 and want[2] != 0, want   # each alone fails a check of its own
                    assert want[3] == number, want


# ---- 4. batch shapes -------------------------------------------------------------------------------------------------------------------
POOL = (4, 2, 2, 8, 3, True, 0, 0)


@pytest.fixture(scope="module")
def pool(zk, orc):
    """The valid proofs and the rejected items of the POOL corpus (SHA-256) with the CPU's numbers, strict and plain."""
    items = verify_ext_corpus.corpus(orc, *POOL, 0)
    cpu = {s: verify_ext_corpus.cpu_checks(zk.load(), items, *POOL, 0, s) for s in (True, False)}
    good = [i for i, it in enumerate(items) if it.label.endswith(".valid")]
    bad = [i for i in range(len(items)) if cpu[False][i] != 0]
    assert len(good) == 2 and (cpu[True][good] == 0).all() and len(set(cpu[False][bad].tolist())) > 5
    return items, cpu, good, bad


@gpu
@pytest.mark.parametrize("count", [5, 65])
def test_batch_shapes_and_strides(zk, pool, count):
    """5 proofs, and 65 (crossing one wave); a stride longer than the proof, the padding noise; a bad proof at index 0, 63, 64 and the
    last, each another rejection, valid proofs everywhere else.  Every element is compared: a rejection never leaks to a neighbour."""
    items, cpu, good, bad = pool
    plen = len(items[0].data)
    idx = np.array([good[r % 2] for r in range(count)])
    places = [at for at in sorted({0, 63, 64, count - 1}) if at < count]
    for n, at in enumerate(places):
        idx[at] = bad[(7 * n + count) % len(bad)]
    rng = np.random.default_rng(count)
    with _verifier(zk, *POOL) as v:
        for extra in (0, 3, 64):
            data = rng.integers(0, 256, (count, plen + extra), dtype=np.uint8)
            for r, i in enumerate(idx):
                data[r, :plen] = np.frombuffer(items[i].data, dtype=np.uint8)
            last = [items[i].public_last for i in idx]
            states = np.stack([np.frombuffer(items[i].state, dtype=np.uint8) for i in idx])
            for strict in (True, False):
                got = v.verify_raw(data, last, states if strict else None)
                assert np.array_equal(got, cpu[strict][idx]), (extra, strict, got, cpu[strict][idx])
                assert np.nonzero(got)[0].tolist() == places


# ---- 5. a proof of the other format ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", ["ext_by_plain", "plain_by_ext"])
def test_a_proof_of_the_other_format(zk, orc, case):
    """(5, 2, q = 2, K = 2, one-value leaves, cap 4): an ext proof read by an ext-off verifier and the reverse, each cut or zero-padded to
    the verifier's length, gets the CPU's number for those bytes (zk_verify_cap with ext off), and Verifier.verify names the difference."""
    lib = zk.load()
    log_n, log_b, q, g, K, coset, D, c = shape = (5, 2, 2, 0, 2, False, 0, 4)
    p_ext, v_ext = (1, 0) if case == "ext_by_plain" else (0, 1)
    if p_ext:
        proofs = verify_ext_corpus.ref_proofs(orc, *shape, 0)
    else:
        proofs = verify_cap_corpus.ref_proofs(orc, *shape, 0)
    with _verifier(zk, *shape, ext_log=v_ext) as v:
        plen = v.proof_len
        assert plen != len(proofs[0][0]) and lib.zk_verifier_get_ext(v._h) == v_ext
        items = [Item(f"{case}.p{i}", (d + bytes(plen))[:plen], s, last) for i, (d, s, last) in enumerate(proofs)]
        for strict in (True, False):
            if v_ext:
                want = verify_ext_corpus.cpu_checks(lib, items, *shape, 0, strict)
            else:
                want = verify_cap_corpus.cpu_checks(lib, items, *shape, 0, strict)
            got = _gpu(v, items, strict, stride=max(plen, len(proofs[0][0])))
            assert (want != 0).all() and np.array_equal(got, want), (case, strict, got, want)
        with pytest.raises(zk.ZkError) as err:
            v.verify([zk.Proof(s, d, log_n, log_b, last, queries=q, fold_log=K, cap_log=c, ext_log=p_ext) for d, s, last in proofs])
        assert "ext_log" in str(err.value)


# ---- 6. one handle between ext off and on ----------------------------------------------------------------------------------------------
@gpu
def test_one_handle_walks_between_ext_off_and_on(zk, orc):
    """ext 0 -> 1 -> 0 -> 1 on one (6, 3) handle with q = 2, while K, the leaf format, D and the cap change as well: each run reads the
    format of the current settings.  With ext off the results are zk_verify_cap's on the plain corpus of those settings."""
    lib = zk.load()
    log_n, log_b, q, g = 6, 3, 2, 0
    walk = [(0, 1, False, 0, 2), (1, 3, True, 2, 4), (0, 3, True, 2, 4), (1, 2, False, 0, 0)]
    with zk.Verifier(log_n, log_b, queries=q) as v:
        for step, (ext, K, coset, D, c) in enumerate(walk):
            if step % 2:                                          # no order between the setters
                v.set_ext(ext); v.set_merkle_cap(c); v.set_fri_stop(D); v.set_fold(K); v.set_coset_leaves(coset)
            else:
                v.set_coset_leaves(coset); v.set_fold(K); v.set_fri_stop(D); v.set_merkle_cap(c); v.set_ext(ext)
            assert lib.zk_verifier_get_ext(v._h) == ext == v.ext_log
            assert v.proof_len == lib.zk_proof_data_len_ext(log_n, log_b, q, g, K, int(coset), D, c, ext)
            mod = verify_ext_corpus if ext else verify_cap_corpus
            items = mod.corpus(orc, log_n, log_b, q, g, K, coset, D, c, 0)
            for strict in (True, False):
                want = mod.cpu_checks(lib, items, log_n, log_b, q, g, K, coset, D, c, 0, strict)
                got = _gpu(v, items, strict)
                assert len(set(want.tolist())) > 5
                assert np.array_equal(got, want), (step, strict, _mismatches(items, got, want))


# ---- 7. round trip -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("log_n,log_b,K,coset", [(10, 3, 3, True), (4, 2, 1, False)])
def test_the_provers_own_proofs(zk, log_n, log_b, K, coset):
    trace = zk.trace_fibsq((1 << log_n) - 1, 1, 3141592)
    with zk.Context(log_n, log_b, queries=2, fold_log=K, coset_leaves=coset, ext_log=1) as ctx:
        pr = ctx.prove(trace)
    assert pr.ext_log == 1 and pr.check(strict=True) == 0
    bad = zk.Proof(pr.state, pr.data[:-1] + bytes([pr.data[-1] ^ 1]), log_n, log_b, pr.public_last, queries=2, fold_log=K, coset_leaves=coset, ext_log=1)
    with zk.Verifier(log_n, log_b, queries=2, fold_log=K, coset_leaves=coset, ext_log=1) as v:
        got = v.verify([pr, bad, pr], strict=True)
        assert got.tolist() == [0, bad.check(strict=True), 0] and got[1] != 0


# ---- 8. refusals on a live handle --------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_setting_and_the_handle_as_they_were(zk, orc):
    lib = zk.load()
    shape = (4, 2, 2, 8, 3, True, 0, 0)
    ext_items = [Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(verify_ext_corpus.ref_proofs(orc, *shape, 0))]
    with _verifier(zk, *shape) as v:
        assert lib.zk_verifier_set_ext(v._h, 2) == -1 and b"zk_verifier_set_ext" in lib.zk_last_error()
        with pytest.raises(zk.ZkError):
            v.set_ext(2)
        assert lib.zk_verifier_get_ext(v._h) == 1 and v.ext_log == 1
        assert lib.zk_verifier_set_shared(v._h, 3, 0) == -1 and b"zk_verifier_set_ext" in lib.zk_last_error()   # names the other setting
        with pytest.raises(zk.ZkError, match="ext"):
            v.set_shared(3)
        with pytest.raises(zk.ZkError):
            v.set_shared(3, True)
        assert lib.zk_verifier_get_shared(v._h) == 0 and v.log_batch == 0 and lib.zk_verifier_get_shared_rows(v._h) == 0
        assert lib.zk_verifier_get_ext(v._h) == 1
        assert lib.zk_verifier_set_shared(v._h, 0, 0) == 0                                                    # plain proofs: nothing to refuse
        assert (_gpu(v, ext_items, True) == 0).all()                                                           # a following run still works
    log_n, log_b, q, g, K, coset, D, c = shape
    with _verifier(zk, *shape, ext_log=0) as v:
        v.set_shared(3)
        assert lib.zk_verifier_set_ext(v._h, 1) == -1 and b"zk_verifier_set_shared" in lib.zk_last_error()     # names the other setting
        with pytest.raises(zk.ZkError, match="shared"):
            v.set_ext(1)
        assert lib.zk_verifier_get_ext(v._h) == 0 and v.ext_log == 0 and lib.zk_verifier_get_shared(v._h) == 3
        assert lib.zk_verifier_set_ext(v._h, 0) == 0                                                            # off stays settable
        v.set_shared(0)
        v.set_ext(1)                                                                                          # and now it is taken
        assert (_gpu(v, ext_items, False) == 0).all()
        plain = [Item(f"p{i}", d, s, last) for i, (d, s, last) in enumerate(verify_cap_corpus.ref_proofs(orc, *shape, 0))]
        v.set_ext(0)
        assert (_gpu(v, plain, True) == 0).all()
    with pytest.raises(zk.ZkError):
        zk.Verifier(log_n, log_b, log_batch=2, ext_log=1)
