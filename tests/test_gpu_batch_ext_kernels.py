"""The kernels of the batch over E on the GPU (zk_dev_compose_ext_batch, zk_dev_fri_fold_multi_ext_batch,
zk_dev_merkle_build_coset_ext_batch), each against kernels that passed their own tests: plane j of proof p of the batched
composition against zk_dev_compose with component j of proof p's alphas, proof p's planes of the batched butterfly against
zk_dev_fri_fold_multi_ext, every node of the heap with coset leaves of E against zk_row_leaf_hash and zk_dev_merkle_build_rows.  Guard
words lie around every output."""
import ctypes as C

import numpy as np
import pytest

from transforms_ref import P, rand_field

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
SPECIAL = (0, 1, P - 1, P, P + 5, 2**32 - 1)                 # raws: the last three are >= P and reduced on the device


@pytest.fixture
def hb():
    from sharded_mirror import HipBackend
    b = HipBackend(0)
    yield b
    b.close()


def _guarded(hb, nwords, aligned=True):
    """A device buffer of nwords with four guard words in front and behind; not aligned: one word past a 16-byte boundary."""
    lead = 4 if aligned else 5
    full = hb.empty(lead + nwords + 4)
    full.fill_(int(np.uint32(GUARD).view(np.int32)))
    body = full[lead:lead + nwords]
    assert (body.data_ptr() % 16 == 0) == aligned
    return full, body, lead


def _guards_intact(hb, full, lead, nwords):
    host = hb.to_host(full)
    return (host[:lead] == GUARD).all() and (host[lead + nwords:] == GUARD).all()


# ---- 1. cp over E of a batch ---------------------------------------------------------------------------------------------------------
# log_blowup 1 and 2 take the window path of the wide form (B < 4), 3 the whole-vector taps; (13, 3) has more than one workgroup per proof
COMPOSE = [(log_n, log_b) for log_n in (3, 4, 5) for log_b in (1, 2, 3)] + [(13, 3)]


@pytest.mark.parametrize("log_n,log_b", COMPOSE, ids=lambda v: str(v))
def test_compose_ext_batch_is_the_base_composition_per_plane(zk, hb, log_n, log_b):
    from zkstark_amd._lib import check
    lib, N = hb.lib, 1 << (log_n + log_b)
    dom = hb.domain(log_n, log_b, 5)
    rng = np.random.default_rng(100 * log_n + log_b)
    f = [rand_field(rng, N) for _ in range(8)]
    f[0][0] = f[7][-1] = P - 1
    first = [int(v) for v in rng.integers(0, P, 8)]
    last = [int(v) for v in rng.integers(0, P, 8)]
    alpha = [[SPECIAL[(p + k) % len(SPECIAL)] if (p + k) % 3 == 0 else int(rng.integers(0, 2**32)) for k in range(6)] for p in range(8)]
    want = {}
    for p in range(8):                                       # plane j of proof p: zk_dev_compose with (alpha0.cj, alpha1.cj, alpha2.cj)
        d_f = hb.upload(f[p])
        for j in (0, 1):
            cp = hb.empty(N)
            hb.compose(dom, d_f, cp, first[p], last[p], [alpha[p][j], alpha[p][2 + j], alpha[p][4 + j]])
            want[p, j] = hb.to_host(cp).copy()
    for nb in (1, 2, 3, 8):
        o = 8 - nb if nb < 8 else 0                          # which proofs of the eight form this batch
        for aligned in (True, False):                        # four values per lane, and the one-value form (no N here is below 16)
            d_f = hb.upload(np.concatenate(f[o:o + nb]))
            full, cp, lead = _guarded(hb, 2 * nb * N, aligned)
            work = hb.empty(12 * nb)
            fi, la = np.array(first[o:o + nb], dtype=np.uint32), np.array(last[o:o + nb], dtype=np.uint32)
            al = np.array(alpha[o:o + nb], dtype=np.uint32)
            check(lib.zk_dev_compose_ext_batch(dom, d_f.data_ptr(), cp.data_ptr(), fi.ctypes.data_as(C.c_void_p), la.ctypes.data_as(C.c_void_p),
                                               al.ctypes.data_as(C.c_void_p), work.data_ptr(), nb, hb._stream()))
            got = hb.to_host(cp).reshape(2, nb, N)
            for p in range(nb):
                for j in (0, 1):
                    assert np.array_equal(got[j, p], want[o + p, j]), (nb, p, j, aligned)
            assert _guards_intact(hb, full, lead, 2 * nb * N), (nb, aligned)


# ---- 2. the butterfly over E of a batch ------------------------------------------------------------------------------------------------
def _fold_ext_one(hb, dom, planes, log_m, rnd, steps, beta):
    from zkstark_amd._lib import check
    src, dst = hb.upload(planes), hb.empty(2 << (log_m - steps))
    check(hb.lib.zk_dev_fri_fold_multi_ext(dom, src.data_ptr(), dst.data_ptr(), log_m, rnd, steps, (C.c_uint32 * 2)(*beta), hb._stream()))
    return hb.to_host(dst).copy()


@pytest.mark.parametrize("rnd", [0, 3])
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_fold_multi_ext_batch_is_the_one_call_fold_per_proof(zk, hb, steps, rnd):
    """q outputs per proof: 1 and 2 take the one-output form with a proof index per lane, 4 is the first wide one, 1024 and 2048 have
    waves inside one proof (constants through scalar loads); one word past alignment sends 1024 through the one-output form as well."""
    from zkstark_amd._lib import check
    lib = hb.lib
    for log_q in (0, 1, 2, 10, 11):
        log_m = log_q + steps
        log_n = log_m + rnd                                  # a fold-only domain without blow-up: layers down to one value per proof
        dom = hb.domain(log_n, 0, 5, fold_only=True)
        m, q = 1 << log_m, 1 << log_q
        rng = np.random.default_rng(1000 * steps + 100 * rnd + log_q)
        planes = [np.concatenate([rand_field(rng, m), rand_field(rng, m)]) for _ in range(8)]
        planes[0][0] = planes[7][-1] = P - 1
        betas = [(SPECIAL[(p + log_q) % len(SPECIAL)], SPECIAL[(p + steps + 3) % len(SPECIAL)]) if p % 2 == 0 else
                 (int(rng.integers(0, 2**32)), int(rng.integers(0, 2**32))) for p in range(8)]
        betas[1] = (2**32 - 1, P + 5)                        # both components >= P in one challenge
        want = [_fold_ext_one(hb, dom, planes[p], log_m, rnd, steps, betas[p]) for p in range(8)]
        for nb in (1, 3, 8):
            o = (log_q + nb) % (8 - nb + 1)
            for aligned in ((True, False) if log_q in (2, 10) else (True,)):
                src = np.concatenate([np.concatenate([planes[p][:m] for p in range(o, o + nb)]), np.concatenate([planes[p][m:] for p in range(o, o + nb)])])
                d_in = hb.upload(src)
                full, out, lead = _guarded(hb, 2 * nb * q, aligned)
                beta = hb.upload(np.array(betas[o:o + nb], dtype=np.uint32).reshape(-1))
                work = hb.empty(24 * nb)
                check(lib.zk_dev_fri_fold_multi_ext_batch(dom, d_in.data_ptr(), out.data_ptr(), log_m, rnd, steps, beta.data_ptr(), work.data_ptr(), nb,
                                                          hb._stream()))
                got = hb.to_host(out).reshape(2, nb, q)
                for p in range(nb):
                    for j in (0, 1):
                        assert np.array_equal(got[j, p], want[o + p][j * q:(j + 1) * q]), (log_q, nb, p, j, aligned, betas[o + p])
                assert _guards_intact(hb, full, lead, 2 * nb * q), (log_q, nb, aligned)


# ---- 3. coset leaves of E over a batch ---------------------------------------------------------------------------------------------------
def _node_bytes(words):
    return words.reshape(-1, 8).astype(">u4").view(np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("h", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_len", [3, 4, 5, 6, 12])
def test_every_node_of_the_heap_with_coset_leaves_of_e(zk, orc, hb, log_len, h):
    """log_len 12 with batch 8 and steps 1 has 2^14 leaves: lanes that make four trips.  Leaf (p, c) is zk_row_leaf_hash of its 2 S
    words; proof p's subtree is zk_dev_merkle_build_rows over its own [2 S][m] array, the tree the one-call prover builds; the nodes above
    the per-proof roots are hashed here from the roots."""
    from zkstark_amd._lib import check
    lib, ln = hb.lib, 1 << log_len
    rng = np.random.default_rng(10 * log_len + h)
    for steps in (1, 2, 3):
        if steps >= log_len:
            continue
        S, log_m = 1 << steps, log_len - steps
        m = 1 << log_m
        for lb in (0, 1, 3):
            nb = 1 << lb
            vals = rng.integers(0, P, (2, nb, ln), dtype=np.uint64).astype(np.uint32)
            vals[:, :, 0], vals[:, nb - 1, -1] = P - 1, 0
            d_vals = hb.upload(vals.reshape(-1))
            total = nb * m
            full, nodes, lead = _guarded(hb, (2 * total - 1) * 8)
            check(lib.zk_dev_merkle_build_coset_ext_batch(d_vals.data_ptr(), log_len, steps, lb, nodes.data_ptr(), hb._stream(), h))
            got = _node_bytes(hb.to_host(nodes))
            assert _guards_intact(hb, full, lead, (2 * total - 1) * 8)
            out = np.zeros(32, dtype=np.uint8)
            for p in range(nb):
                # this proof's [2 S][m] array: row plane * S + u holds slot u of every leaf
                rows = np.concatenate([vals[j, p].reshape(S, m) for j in (0, 1)])
                for c in range(m):
                    words = np.ascontiguousarray(rows[:, c])
                    assert lib.zk_row_leaf_hash(words.ctypes.data_as(C.c_void_p), 2 * S, h, out.ctypes.data_as(C.c_void_p)) == 0
                    assert np.array_equal(got[total - 1 + p * m + c], out), (steps, lb, p, c)
                d_rows = hb.upload(rows.reshape(-1))
                sub = hb.empty((2 * m - 1) * 8)
                check(lib.zk_dev_merkle_build_rows(d_rows.data_ptr(), log_m, steps + 1, sub.data_ptr(), hb._stream(), h))
                want = _node_bytes(hb.to_host(sub))
                for d in range(log_m + 1):
                    a = (1 << (lb + d)) - 1 + (p << d)
                    assert np.array_equal(got[a:a + (1 << d)], want[(1 << d) - 1:(2 << d) - 1]), (steps, lb, p, d)
            orc.set_hash(h)
            try:
                for i in range(nb - 2, -1, -1):               # the lb levels above the per-proof roots
                    assert bytes(got[i]) == orc.node_hash(bytes(got[2 * i + 1]), bytes(got[2 * i + 2])), (steps, lb, i)
            finally:
                orc.set_hash(0)


def test_the_probes_refuse_bad_shapes(zk, hb):
    lib = hb.lib
    dom = hb.domain(4, 1, 5)
    buf, odd = hb.empty(256), hb.empty(64)[1:]
    one = np.ones(6, dtype=np.uint32)
    hp = one.ctypes.data_as(C.c_void_p)
    assert lib.zk_dev_compose_ext_batch(dom, buf.data_ptr(), buf.data_ptr(), hp, hp, hp, buf.data_ptr(), 0, hb._stream()) == -1
    assert lib.zk_dev_compose_ext_batch(dom, buf.data_ptr(), buf.data_ptr(), hp, hp, hp, odd.data_ptr(), 1, hb._stream()) == -1      # d_work alignment
    for steps, rnd, nb in ((0, 0, 1), (4, 0, 1), (2, 3, 1), (1, 0, 0)):
        assert lib.zk_dev_fri_fold_multi_ext_batch(dom, buf.data_ptr(), buf.data_ptr(), 5 - rnd, rnd, steps, buf.data_ptr(), buf.data_ptr(), nb, hb._stream()) == -1
    assert lib.zk_dev_fri_fold_multi_ext_batch(dom, buf.data_ptr(), buf.data_ptr(), 5, 0, 1, buf.data_ptr(), odd.data_ptr(), 1, hb._stream()) == -1
    for log_len, steps, lb, kind in ((3, 0, 1, 0), (3, 3, 1, 0), (3, 4, 1, 0), (28, 1, 3, 0), (4, 1, 1, 2)):
        assert lib.zk_dev_merkle_build_coset_ext_batch(buf.data_ptr(), log_len, steps, lb, buf.data_ptr(), hb._stream(), kind) == -1
