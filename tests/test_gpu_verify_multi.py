"""The batched GPU verifier held to the CPU's FIRST failure (zk_verifier_run; verify.hip): every element of checks_out is the number
the CPU verifier stops at when a proof has several faults (tests/verify_multi_corpus.py: every pair of fault classes, and triples,
in the three wire formats and their three order-key schemes), for seeded random mutations of valid proofs, across the chunks of a
batch larger than one chunk (by count and by bytes), on a handle whose buffers grow and are reused, and in a wave whose lanes leave
by every exit (accepted, an order key, the malformed re-run, the transcript)."""
import time

import numpy as np
import pytest

import verify_corpus
import verify_multi_corpus as mc

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
P = verify_corpus.P


def _shape_id(shape):
    return "-".join(str(x) for x in shape)


def _verifier(zk, shape, hash_kind):
    fmt, log_n, log_b, q, g, K = shape
    return zk.Verifier(log_n, log_b, hash=HASH_NAMES[hash_kind], queries=q, grind_bits=g, fold_log=K, coset_leaves=fmt == "coset")


def _gpu(v, items, strict, order=None):
    order = range(len(items)) if order is None else order
    data = np.stack([np.frombuffer(items[i].data, dtype=np.uint8) for i in order])
    states = np.stack([np.frombuffer(items[i].state, dtype=np.uint8) for i in order]) if strict else None
    return v.verify_raw(data, [items[i].public_last for i in order], states)


def _mismatches(items, got, want):
    return [(items[i].label, int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", mc.SHAPES, ids=_shape_id)
def test_checks_equal_the_cpu_on_the_multi_fault_corpus(zk, orc, shape, hash_kind):
    """Singles, pairs and triples of faults in one call, strict and plain, on one Verifier: element for element the CPU's number.
    What the corpus distinguishes is asserted without a GPU in tests/test_verify_multi_corpus.py."""
    c = mc.corpus(orc, *shape, hash_kind)
    with _verifier(zk, shape, hash_kind) as v:
        assert v.proof_len == len(c.items[0].data)
        for strict in (True, False):
            want = mc.cpu_numbers(zk.load(), orc, shape, hash_kind, strict)
            t = time.perf_counter()
            got = _gpu(v, c.items, strict)
            print(f"shape {shape} {HASH_NAMES[hash_kind]} strict {strict}: {len(c.items)} items, {len(set(want.tolist()))} distinct check numbers, "
                  f"{(got != want).sum()} mismatches, {time.perf_counter() - t:.2f} s on the device")
            assert got.shape == want.shape
            assert np.array_equal(got, want), (strict, _mismatches(c.items, got, want))


# ---- seeded random mutations ---------------------------------------------------------------------------------------------------
MUTATION_SHAPES = [("plain", 10, 3, 1, 0, 1), ("fold", 7, 1, 2, 0, 3), ("coset", 10, 3, 2, 8, 2)]
MUTANTS, INPUT_MUTANTS = 1500, 20


def _mutants(orc, shape, hash_kind):
    """1 500 mutants of the two valid proofs: 1..4 words at uniformly random word offsets (counts and the nonce included), each a
    one-bit flip, a random word or + P where that fits a u32; then 20 that change only public_last or the state.  Returns the
    items and the set of (path length, level) of every altered digest."""
    proofs = mc.valid_proofs(orc, *shape, hash_kind)
    rng = np.random.default_rng([20240612, hash_kind] + list(shape[1:]))
    words = len(proofs[0][0]) // 4
    regions = [mc.path_regions(*shape, d) for d, _, _ in proofs]
    items, levels = [], set()
    for m in range(MUTANTS):
        p = m % len(proofs)
        data, state, last = proofs[p]
        w = np.frombuffer(data, dtype="<u4").copy()
        how = []
        for off in rng.integers(0, words, int(rng.integers(1, 5))):
            kind = int(rng.integers(0, 3))
            old = int(w[off])
            if kind == 2 and old + P >= 2**32:
                kind = 0
            w[off] = old ^ (1 << int(rng.integers(0, 32))) if kind == 0 else int(rng.integers(0, 2**32)) if kind == 1 else old + P
            how.append(f"{int(off)}{'^r+'[kind]}")
            if int(w[off]) != old:
                for start, n in regions[p]:
                    if start <= 4 * off < start + 32 * n:
                        levels.add((n, (4 * int(off) - start) // 32))
        items.append(verify_corpus.Item(f"p{p}.m{m}." + ",".join(how), w.tobytes(), state, last))
    for m in range(INPUT_MUTANTS):
        data, state, last = proofs[m % len(proofs)]
        if m % 2:
            st = bytearray(state)
            st[int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
            items.append(verify_corpus.Item(f"input{m}.state", data, bytes(st), last))
        else:
            new = (last ^ (1 << int(rng.integers(0, 32))), last + 1, int(rng.integers(0, 2**32)))[(m // 2) % 3]
            items.append(verify_corpus.Item(f"input{m}.public_last", data, state, new))
    return items, levels


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_shape_id)
def test_checks_equal_the_cpu_on_random_mutations(zk, orc, shape, hash_kind):
    """Nothing here is chosen by hand: every path level of every path length is altered somewhere, counts are hit now and then
    (the malformed re-run, also with a count that stays plausible), and most mutants carry several faults."""
    items, levels = _mutants(orc, shape, hash_kind)
    cpu = {s: mc.cpu_checks(zk.load(), items, *shape, hash_kind, s) for s in (True, False)}
    plain = cpu[False][:MUTANTS]
    lengths = {n for _, n in mc.path_regions(*shape, items[0].data)}
    print(f"shape {shape} {HASH_NAMES[hash_kind]}: {(plain == 0).sum()} of {MUTANTS} accepted in plain mode, {len(set(plain.tolist()))} distinct "
          f"check numbers, {len(levels)} (length, level) pairs altered, path lengths {sorted(lengths)}")
    # conditions on the corpus, from the CPU numbers alone: the unused root of the last layer is about 0.4 % of the bytes, and a
    # challenge + P is accepted in plain mode
    assert (plain == 0).sum() <= 0.02 * MUTANTS
    assert len(set(plain.tolist())) >= 8
    assert levels == {(n, lvl) for n in lengths for lvl in range(n)}
    with _verifier(zk, shape, hash_kind) as v:
        for strict in (True, False):
            t = time.perf_counter()
            got = _gpu(v, items, strict)
            print(f"  strict {strict}: {(got != cpu[strict]).sum()} mismatches, {time.perf_counter() - t:.2f} s on the device")
            assert np.array_equal(got, cpu[strict]), (strict, _mismatches(items, got, cpu[strict]))


# ---- chunks --------------------------------------------------------------------------------------------------------------------
CHUNK_PROOFS = 65536                  # zk_verifier_run: a chunk is at most 2^16 proofs ...
CHUNK_BYTES = 256 << 20               # ... and at most 256 MiB of proof bytes


@pytest.fixture(scope="module")
def small_pool(zk, orc):
    """The single-fault corpus of the plain (2, 1) format (956 bytes a proof), shuffled: the items as arrays and the CPU's numbers."""
    items = verify_corpus.corpus(orc, 2, 1, 1, 0)
    items = [items[i] for i in np.random.default_rng(11).permutation(len(items))]
    cpu = {s: mc.cpu_checks(zk.load(), items, "plain", 2, 1, 1, 0, 1, 0, s) for s in (True, False)}
    data = np.stack([np.frombuffer(it.data, dtype=np.uint8) for it in items])
    states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in items])
    last = np.array([it.public_last for it in items], dtype=np.uint32)
    return items, data, states, last, cpu


def _run_pool(v, pool, idx, strict, extra=0):
    items, data, states, last, cpu = pool
    rows = data[idx]
    if extra:
        rows = np.concatenate([rows, np.full((len(idx), extra), 0xA5, dtype=np.uint8)], axis=1)
    got = v.verify_raw(rows, last[idx], states[idx] if strict else None)
    bad = [(int(i), items[idx[i]].label, int(got[i]), int(cpu[strict][idx[i]])) for i in np.nonzero(got != cpu[strict][idx])[0][:20]]
    assert not bad, (strict, extra, bad)


def test_more_proofs_than_one_chunk(zk, small_pool):
    """65 536 + 1 000 proofs: the second iteration of the chunk loop (proofs + i stride, states + 32 i, public_last + i,
    checks_out + i for i > 0), a last chunk smaller than the buffers, the per-proof results set up again.  The last proof of chunk 0
    and the first of chunk 1 are rejected at different checks and their outer neighbours are accepted."""
    items, _, _, _, cpu = small_pool
    assert len(items[0].data) == 956
    n = CHUNK_PROOFS + 1000
    idx = np.arange(n) % len(items)
    rejected = [i for i in range(len(items)) if cpu[True][i] and cpu[False][i]]
    accepted = [i for i in range(len(items)) if not cpu[True][i] and not cpu[False][i]]
    r0 = rejected[0]
    r1 = next(i for i in rejected if cpu[False][i] != cpu[False][r0] and cpu[True][i] != cpu[True][r0])
    idx[CHUNK_PROOFS - 2:CHUNK_PROOFS + 2] = [accepted[0], r0, r1, accepted[0]]
    with zk.Verifier(2, 1) as v:
        assert v.proof_len == 956
        for extra in (0, 3):
            for strict in (True, False):
                _run_pool(v, small_pool, idx, strict, extra)


def test_more_bytes_than_one_chunk(zk, orc):
    """q = 64: a proof of (5, 2) is about 170 KB, so 256 MiB of proof bytes end a chunk after about 1 600 proofs.  A few proofs
    more than that, strict, with tampered proofs on both sides of the boundary and a wrong state at the very end."""
    log_n, log_b, q = 5, 2, 64
    with zk.Verifier(log_n, log_b, queries=q) as v:
        plen = v.proof_len
        chunk = CHUNK_BYTES // plen
        assert 1 < chunk < CHUNK_PROOFS
        proofs = verify_corpus.oracle_proofs(orc, log_n, log_b, q, 0)
        assert len(proofs[0][0]) == plen
        fields = {name: off for name, off, _, _ in verify_corpus.fields(log_n, log_b, q)}
        pool = [verify_corpus.Item(f"p{i}.valid", d, s, last) for i, (d, s, last) in enumerate(proofs)]
        for i, name, bit in ((0, "q63.layer4.nx", 3), (1, "alpha2", 9), (0, "q31.f1.value", 30), (1, "beta3", 0)):
            d, s, last = proofs[i]
            b = bytearray(d)
            b[fields[name] + bit // 8] ^= 1 << (bit % 8)
            pool.append(verify_corpus.Item(f"p{i}.{name}", bytes(b), s, last))
        pool.append(verify_corpus.Item("p0.state", proofs[0][0], bytes(32), proofs[0][2]))
        pool.append(verify_corpus.Item("p1.public_last", proofs[1][0], proofs[1][1], proofs[1][2] + 1))
        want = mc.cpu_checks(zk.load(), pool, "plain", log_n, log_b, q, 0, 1, 0, True)
        assert want[:2].tolist() == [0, 0] and (want[2:] != 0).all() and len(set(want.tolist())) >= 5
        count = chunk + 5
        idx = np.arange(count) % len(pool)
        idx[chunk - 3:chunk + 3] = [0, 2, 3, 4, 7, 1]        # ..., valid, tampered, tampered | tampered, wrong public_last, valid, ...
        idx[count - 1] = 6                                   # the wrong state
        data = np.stack([np.frombuffer(it.data, dtype=np.uint8) for it in pool])[idx]
        assert data.nbytes > CHUNK_BYTES
        states = np.stack([np.frombuffer(it.state, dtype=np.uint8) for it in pool])[idx]
        got = v.verify_raw(data, np.array([it.public_last for it in pool], dtype=np.uint32)[idx], states)
        bad = [(int(i), pool[idx[i]].label, int(got[i]), int(want[idx[i]])) for i in np.nonzero(got != want[idx])[0][:20]]
        assert not bad, bad


def test_one_handle_across_small_and_large_batches(zk, orc, small_pool):
    """3, 70 000, 5, 70 000 proofs on one handle, each a different rotation of the pool: the buffers grow once and are reused, and
    a small run after a large one sees nothing of the large one's results.  Then the handle's query count changes, so the proofs
    grow, and it runs once more."""
    items = small_pool[0]
    with zk.Verifier(2, 1) as v:
        for count, rot in ((3, 0), (70000, 17), (5, 41), (70000, 59)):
            idx = (np.arange(count) + rot) % len(items)
            for strict in (True, False):
                _run_pool(v, small_pool, idx, strict)
        before = v.proof_len
        assert zk.load().zk_verifier_set_queries(v._h, 3) == 0
        v.queries = 3
        assert v.proof_len > before
        q3 = verify_corpus.corpus(orc, 2, 1, 3, 0)
        for strict in (True, False):
            want = mc.cpu_checks(zk.load(), q3, "plain", 2, 1, 3, 0, 1, 0, strict)
            got = _gpu(v, q3, strict)
            assert np.array_equal(got, want), (strict, _mismatches(q3, got, want))


# ---- a wave of mixed exits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [("fold", 5, 2, 3, 8, 2), ("coset", 5, 2, 3, 8, 2)], ids=_shape_id)
def test_one_wave_of_mixed_exits(zk, orc, shape):
    """64 proofs in one call, so one workgroup of the paths and transcript kernels holds all of them: 16 accepted, 16 that fail an
    order key, 16 malformed (the host's re-run) and 16 that fail the transcript in strict mode.  The tampered proofs are pairs of
    the multi-fault corpus; those of the second and third kind carry the state of their own bytes (mc.transcript_state), so the
    strict replay passes and strict mode reaches the key and the re-run as well.  Order fixed by a seed, then reversed."""
    c = mc.corpus(orc, *shape, 0)
    rng = np.random.default_rng(64)
    kinds = lambda p, a, b: {c.classes[p][a].kind, c.classes[p][b].kind}                    # noqa: E731
    keyed = [i for i, p, a, b in c.pairs if kinds(p, a, b) <= {"algebra", "paths"}]
    plain = mc.cpu_numbers(zk.load(), orc, shape, 0, False)                                 # a count the CPU stops at, not one it never reaches
    counted = [i for i, p, a, b in c.pairs if "count" in kinds(p, a, b) and "global" not in kinds(p, a, b) and plain[i] == -1]
    heads = [i for i, p, a, b in c.pairs if "global" in kinds(p, a, b) and c.classes[p][a].name != "public_last" and c.classes[p][b].name != "public_last"]
    items = [c.items[c.valid[i % 2]] for i in range(16)]
    for i in list(rng.choice(keyed, 16, replace=False)) + list(rng.choice(counted, 16, replace=False)):
        it = c.items[i]
        items.append(verify_corpus.Item(it.label + "|restated", it.data, mc.transcript_state(shape[0], it.data, *shape[1:]), it.public_last))
    items += [c.items[i] for i in rng.choice(heads, 16, replace=False)]
    cpu = {s: mc.cpu_checks(zk.load(), items, *shape, 0, s) for s in (True, False)}
    print(f"shape {shape}: strict {sorted(set(cpu[True].tolist()))}, plain {sorted(set(cpu[False].tolist()))}")
    # the four exits, from the CPU numbers alone
    assert (cpu[True][:16] == 0).all() and (cpu[False][:16] == 0).all()
    for s in (True, False):
        assert all(c_ in (-2, -4, -5, -6, -7) or -500 < c_ <= -300 or -200 < c_ <= -100 for c_ in cpu[s][16:32]), cpu[s][16:32]
        assert all(c_ in (-1, -3) or -300 < c_ <= -200 for c_ in cpu[s][32:48]), cpu[s][32:48]
    assert (cpu[True][48:] <= -1000).all()
    order = rng.permutation(64)
    with _verifier(zk, shape, 0) as v:
        for o in (order, order[::-1]):
            for strict in (True, False):
                got = _gpu(v, items, strict, o)
                picked = [items[i] for i in o]
                assert np.array_equal(got, cpu[strict][o]), (strict, _mismatches(picked, got, cpu[strict][o]))
