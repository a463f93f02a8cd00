"""Batched verification of shared proofs on the GPU (zk_verifier_set_shared, Verifier(log_batch=, shared_rows=)): every element of
checks_out is the number the CPU verifier zk_verify_shared_rows gives that proof -- for batches of valid proofs built without the library
(tests/shared_ref.py, tests/rows_ref.py), for the tamper corpus of tests/verify_shared_corpus.py, for two broken paths whose order decides
the number, for proofs of another format, and for one handle whose format changes between runs; then one round trip from the library's
prover."""
import numpy as np
import pytest

import verify_cap_corpus
import verify_shared_corpus as vsc

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
CASES = [pytest.param(s, rows, id=vsc.shape_id(s) + ("-rows" if rows else "-plain")) for s in vsc.SHAPES for rows in s[10]]


def _verifier(zk, shape, rows):
    log_n, log_b, lb, K, coset, D, c, q, h, g = shape[:10]
    return zk.Verifier(log_n, log_b, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c,
                       log_batch=lb, shared_rows=rows)


def _gpu(v, items, strict, stride=None, flat=False):
    plen = len(items[0].data)
    data = np.zeros((len(items), stride or plen), dtype=np.uint8)
    for r, it in enumerate(items):
        data[r, :plen] = np.frombuffer(it.data, dtype=np.uint8)
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items]) if strict else None
    last = np.array([it.public_last for it in items], dtype=np.uint32)
    return v.verify_raw(data, last.reshape(-1) if flat else last, states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


@pytest.mark.parametrize("shape,rows", CASES)
def test_valid_batches(zk, orc, shape, rows):
    """5 and 65 proofs (neither the proofs nor the statements of a batch fill whole waves), the last one with a byte of its last path
    flipped: the CPU accepts all but the last, and the GPU agrees, strict and not, also with a stride larger than the proof."""
    lib = zk.load()
    with _verifier(zk, shape, rows) as v:
        assert lib.zk_verifier_get_shared(v._h) == shape[2] and lib.zk_verifier_get_shared_rows(v._h) == int(rows)
        for count in (5, 65):
            items = vsc.valid_batch(orc, shape, rows, count)
            assert v.proof_len == len(items[0].data)
            for strict in (True, False):
                cpu = np.zeros(count, dtype=np.int32)     # the two valid proofs in turn: the CPU checks each once, and the broken one
                first = vsc.cpu_checks(lib, items[:2] + items[-1:], shape, rows, strict)
                cpu[-1] = first[2]
                assert first[0] == 0 and first[1] == 0 and first[2] != 0, first
                got = _gpu(v, items, strict)
                assert np.array_equal(got, cpu), (count, strict, _mismatches(items, got, cpu))
                got = _gpu(v, items, strict, stride=len(items[0].data) + 12, flat=True)
                assert np.array_equal(got, cpu), (count, strict, "stride", _mismatches(items, got, cpu))


@pytest.mark.parametrize("shape,rows", CASES)
def test_checks_equal_the_cpu_on_the_tamper_corpus(zk, orc, shape, rows):
    """The exactness claim: for every element of the corpus, strict and not, checks_out[i] == zk_verify_shared_rows's number; and the corpus
    reaches the checks it is meant to reach."""
    items = vsc.corpus(orc, shape, rows)
    coset = shape[4]
    seen = []
    with _verifier(zk, shape, rows) as v:
        for strict in (True, False):
            want = vsc.cpu_checks(zk.load(), items, shape, rows, strict)
            got = _gpu(v, items, strict)
            print(f"shape {vsc.shape_id(shape)} rows {rows} strict {strict}: {len(items)} items, {(want != 0).sum()} rejected, "
                  f"{sorted(set(want.tolist()))} check numbers, {(got != want).sum()} mismatches")
            assert np.array_equal(got, want), (strict, _mismatches(items, got, want))
            seen += want.tolist()
    assert not vsc.expected_numbers(seen, coset), (vsc.expected_numbers(seen, coset), sorted(set(seen)))


def _flip(data, regs, name):
    off, size = next((o, n) for r, o, n in regs if r == name)
    d = bytearray(data)
    d[off + size - 1] ^= 0x20
    return bytes(d)


def test_first_failure_in_wire_order(zk, orc):
    """One plain shared proof of 8 statements and 2 queries.  The paths of statement 5's f(gx) and of statement 2's f(g^2 x) broken in query 0:
    statement 2 comes first on the wire, -6.  The same two in query 1 and the cp0 relation of query 0 (a changed f value): -2."""
    shape = vsc.SHAPES[1]
    assert shape[2] == 3 and shape[7] == 2
    lib = zk.load()
    data, state, last = vsc.ref_proofs(orc, shape, False)[0]
    regs = vsc.regions(shape, False)
    a = _flip(_flip(data, regs, "q0.s5.f1.path"), regs, "q0.s2.f2.path")
    b = _flip(_flip(_flip(data, regs, "q1.s5.f1.path"), regs, "q1.s2.f2.path"), regs, "q0.s0.f0.value")
    c = _flip(data, regs, "q1.s5.f1.path")
    items = [vsc.Item("q0.s5.f1+q0.s2.f2", a, state, last), vsc.Item("q1.s5.f1+q1.s2.f2+q0.cp0", b, state, last), vsc.Item("q1.s5.f1", c, state, last),
             vsc.Item("valid", data, state, last)]
    with _verifier(zk, shape, False) as v:
        want = vsc.cpu_checks(lib, items, shape, False, False)
        assert want.tolist() == [-6, -2, -5, 0]
        got = _gpu(v, items * 17, False)                   # 68 proofs: the same answers in every wave
        assert np.array_equal(got, np.tile(want, 17)), got
        want = vsc.cpu_checks(lib, items, shape, False, True)
        got = _gpu(v, items, True)
        assert np.array_equal(got, want), (got, want)


def test_proofs_of_another_format(zk, orc):
    """Bytes of one format cut or zero-padded to the length of a verifier of another: the number zk_verify_shared_rows of the verifier's
    settings gives those bytes.  A rows proof read as plain shared and the reverse, a shared proof read at another lb, a plain proof read by
    a shared verifier; Verifier.verify names the setting."""
    lib = zk.load()
    shape = vsc.SHAPES[1]
    log_n, log_b, lb, K, coset, D, c, q, h, g = shape[:10]
    single = verify_cap_corpus.ref_proofs(orc, log_n, log_b, q, g, K, coset, D, c, h)
    sources = {"rows": vsc.ref_proofs(orc, shape, True), "plain": vsc.ref_proofs(orc, shape, False), "single": [(d, s, [last]) for d, s, last in single]}
    for src, v_lb, v_rows in (("rows", lb, False), ("plain", lb, True), ("plain", lb + 1, False), ("rows", lb - 1, True), ("single", lb, False),
                              ("single", 1, True)):
        vshape = shape[:2] + (v_lb,) + shape[3:]
        with _verifier(zk, vshape, v_rows) as v:
            plen, M = v.proof_len, 1 << v_lb
            assert plen != len(sources[src][0][0])
            items = [vsc.Item(f"{src}{i}", (d + bytes(plen))[:plen], s, (last * M)[:M]) for i, (d, s, last) in enumerate(sources[src])]
            for strict in (True, False):
                want = vsc.cpu_checks(lib, items, vshape, v_rows, strict)
                got = _gpu(v, items, strict)
                assert (want != 0).all() and np.array_equal(got, want), (src, v_lb, v_rows, strict, got, want)
    kw = dict(hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c)
    d, s, last = sources["rows"][0]
    with _verifier(zk, shape, False) as v:
        with pytest.raises(zk.ZkError) as err:
            v.verify([zk.SharedProof(s, d, log_n, log_b, lb, last, shared_rows=True, **kw)])
        assert "shared_rows" in str(err.value)
        with pytest.raises(zk.ZkError) as err:
            v.verify([zk.Proof(single[0][1], single[0][0], log_n, log_b, single[0][2], **kw)])
        assert "log_batch" in str(err.value)
        with pytest.raises(zk.ZkError):
            v.verify_raw(np.zeros((2, v.proof_len), dtype=np.uint8), [0, 0])


def test_one_handle_walks_the_shared_settings(zk, orc):
    """lb 0 -> 3 -> 3 with rows -> 0 -> 8 with rows on one handle, K = 3, coset leaves, D = 2, c = 4: every run reads the current format, a
    refused setting leaves the one before in place, and at lb = 0 the results are those of a fresh verifier."""
    lib = zk.load()
    log_n, log_b, K, coset, D, c, q, h = 5, 2, 3, True, 2, 4, 2, 0
    kw = dict(queries=q, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c)
    assert lib.zk_verifier_set_shared(None, 1, 0) == -1 and lib.zk_verifier_get_shared(None) == 0 and lib.zk_verifier_get_shared_rows(None) == 0
    with zk.Verifier(log_n, log_b, **kw) as v:
        for lb, rows in ((0, False), (3, False), (3, True), (0, False), (8, True)):
            v.set_shared(lb, rows)
            for bad in ((9, 0), (0, 1), (9, 1)):
                assert lib.zk_verifier_set_shared(v._h, *bad) == -1
            assert lib.zk_verifier_get_shared(v._h) == lb == v.log_batch and lib.zk_verifier_get_shared_rows(v._h) == int(rows)
            shape = (log_n, log_b, lb, K, coset, D, c, q, h, 0)
            if lb == 0:
                proofs = verify_cap_corpus.ref_proofs(orc, log_n, log_b, q, 0, K, coset, D, c, h)
                items = [vsc.Item(f"p{i}", d, s, [last]) for i, (d, s, last) in enumerate(proofs)]
                d = bytearray(items[0].data)
                d[-5] ^= 4
                items.append(vsc.Item("p0.bad", bytes(d), items[0].state, items[0].public_last))
            else:
                items = vsc.valid_batch(orc, shape, rows, 5) + vsc.corpus(orc, shape, rows)[:40]
            assert v.proof_len == len(items[0].data)
            for strict in (True, False):
                want = vsc.cpu_checks(lib, items, shape, rows, strict)
                got = _gpu(v, items, strict)
                assert np.array_equal(got, want), (lb, rows, strict, _mismatches(items, got, want))
                assert (want == 0).any() and (want != 0).any()
                if lb == 0:
                    with zk.Verifier(log_n, log_b, **kw) as fresh:
                        assert np.array_equal(_gpu(fresh, items, strict), got)


@pytest.mark.parametrize("rows", [False, True], ids=["plain", "rows"])
def test_prover_to_verifier_round_trip(zk, rows):
    """(10, 3), 8 statements, three queries, K = 2, coset leaves, c = 5: what BatchContext.prove_shared makes four times over, Verifier.verify
    accepts, strict and not, and a flipped byte in one proof is that proof's rejection alone, with SharedProof.check's number."""
    log_n, log_b, lb = 10, 3, 3
    kw = dict(queries=3, fold_log=2, coset_leaves=True, cap_log=5)
    with zk.BatchContext(log_n, log_b, log_batch=lb, shared_rows=rows, **kw) as b, zk.Verifier(log_n, log_b, log_batch=lb, shared_rows=rows, **kw) as v:
        proofs = []
        for r in range(4):
            b.gen_fibsq([1] * (1 << lb), [3141592 + 8 * r + p for p in range(1 << lb)])
            proofs.append(b.prove_shared())
        assert all(p.shared_rows == rows and p.check(strict=True) == 0 for p in proofs)
        for strict in (True, False):
            assert (v.verify(proofs, strict=strict) == 0).all()
        d = bytearray(proofs[2].data)
        d[len(d) // 2] ^= 1
        bad = zk.SharedProof(proofs[2].state, bytes(d), log_n, log_b, lb, proofs[2].public_last, shared_rows=rows, **kw)
        got = v.verify([proofs[0], proofs[1], bad, proofs[3]])
        assert got[2] == bad.check(strict=True) != 0 and (got[[0, 1, 3]] == 0).all(), got
