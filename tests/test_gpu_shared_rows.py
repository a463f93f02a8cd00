"""Row leaves of the shared proof on the GPU (zk_batch_set_shared_rows, zk_dev_merkle_build_rows): every node of the tree
row_leaf_hash_kernel and the inner build make against the model of tests/rows_ref.py, the shared proof with row leaves byte for byte
against that model crossed with every setting, one live batch that alternates zk_batch_prove and both kinds of shared proof, a broken
trace, the refusals."""
import ctypes as C
import threading

import numpy as np
import pytest

import cap_ref
import rows_ref
import shared_ref

pytestmark = pytest.mark.gpu

HASH_NAMES = {0: "sha256", 1: "field"}
ERR_INVALID, ERR_STATE, ERR_BUFFER, ERR_CHECK = -1, -4, -5, -7
SEED = rows_ref.SEED

# launch_merkle_build_rows gives every leaf a lane of its own up to 4 * 256 leaves and four leaves to a lane above that: 2^11 leaves is
# the smallest tree in which a lane makes more than one trip (512 lanes, 4 trips each)
FIRST_MULTI_TRIP_LOG = 11
# (log_len, log_batch): N = 8 is fewer leaves than a wave; lb 1 / 3 one compression, 4 the first streamed leaf, 8 the longest
TREES = [(3, 1), (3, 3), (3, 4), (3, 8), (13, 3), (13, 4), (13, 8), (FIRST_MULTI_TRIP_LOG, 4)]


def _seeds(batch):
    return [1] * batch, [SEED + p for p in range(batch)]


@pytest.mark.parametrize("h", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("log_len,lb", TREES, ids=lambda v: str(v))
def test_every_node_of_the_row_tree(zk, orc, log_len, lb, h):
    import torch
    lib = zk.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 * log_len + 10 * lb + h)
    f = rng.integers(0, rows_ref.P, (1 << lb, 1 << log_len), dtype=np.uint64).astype(np.uint32)
    f[:, 0], f[:, -1] = rows_ref.P - 1, 0                   # the largest residue in every slot of a leaf, and an all-zero row
    orc.set_hash(h)
    try:
        want = rows_ref.rows_tree(orc, f, h)
    finally:
        orc.set_hash(0)
    d_vals = torch.from_numpy(f.view(np.int32).copy()).to(dev)
    d_nodes = torch.zeros(((2 << log_len) - 1) * 8, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.zk_dev_merkle_build_rows(d_vals.data_ptr(), log_len, lb, d_nodes.data_ptr(), stream, h) == 0, lib.zk_last_error()
    torch.cuda.current_stream(dev).synchronize()
    got = d_nodes.cpu().numpy().view(np.uint32).reshape(-1, 8).astype(">u4").view(np.uint8).reshape(-1, 32)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {len(want)} nodes differ, first at {bad[:4]}", log_len, lb, h)


def test_row_tree_refusals(zk):
    import torch
    lib = zk.load()
    dev = torch.device("cuda", 0)
    d_vals = torch.zeros(64, dtype=torch.int32, device=dev)
    d_nodes = torch.zeros(15 * 8, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for log_len, lb, kind in ((3, 0, 0), (3, 9, 0), (0, 3, 0), (25, 6, 0), (3, 3, 2), (3, 3, -1)):
        assert lib.zk_dev_merkle_build_rows(d_vals.data_ptr(), log_len, lb, d_nodes.data_ptr(), stream, kind) == ERR_INVALID
    torch.cuda.current_stream(dev).synchronize()
    assert not d_nodes.any().item()                          # nothing was launched


def _same(got, ref, lib, s):
    log_n, log_b, lb, K, coset, D, c, q, g, h = s
    assert got.shared_rows
    assert len(got.data) == len(ref.data) == lib.zk_proof_data_len_shared_rows(log_n, log_b, q, g, K, int(coset), D, c, lb, 1) == got.expected_len()
    assert got.data == ref.data, "proof bytes"
    assert got.state == ref.state and list(got.public_last) == list(ref.public_last)
    assert got.check(strict=True) == 0 and got.check() == 0
    got.verify(strict=True)


# (log_n, log_b, lb, K, coset, D, c, q, grind, hash), host levels to run (None: the default), whose bytes must agree
#   (2,1,*)   L = 3: eight rows, caps 4 and 8 clamp to depth 2 and leave paths of one digest
#   (4,2,*)   L = 6: one wave of rows; the early stop D = 2 fits
#   (10,3,*)  L = 13: four trips per lane, the host's share of the tree top (host levels 1, SHA-256)
CASES = [
    ((2, 1, 1, 1, False, 0, 0, 1, 0, 0), (None,)),
    ((2, 1, 1, 1, False, 0, 8, 1, 0, 1), (None,)),
    ((2, 1, 3, 3, True, 0, 4, 16, 0, 0), (None,)),
    ((2, 1, 4, 1, False, 0, 0, 1, 0, 1), (None,)),
    ((2, 1, 4, 3, True, 0, 8, 1, 8, 0), (0,)),
    ((2, 1, 8, 1, False, 0, 0, 16, 0, 0), (None,)),
    ((2, 1, 8, 3, True, 0, 4, 1, 0, 1), (None,)),
    ((4, 2, 1, 3, True, 2, 0, 1, 0, 0), (1,)),
    ((4, 2, 3, 1, False, 0, 4, 1, 0, 1), (None,)),
    ((4, 2, 3, 3, False, 2, 8, 16, 0, 0), (1, 0)),
    ((4, 2, 4, 1, True, 0, 0, 1, 0, 0), (None,)),
    ((4, 2, 4, 3, True, 2, 4, 1, 8, 1), (None,)),
    ((4, 2, 4, 1, False, 0, 8, 16, 0, 0), (0,)),
    ((4, 2, 8, 3, True, 2, 0, 1, 0, 0), (None,)),
    ((4, 2, 8, 1, False, 0, 4, 1, 0, 1), (None,)),
    ((4, 2, 8, 3, False, 0, 8, 1, 0, 0), (1,)),
    ((10, 3, 1, 1, False, 0, 0, 1, 0, 0), (1, 0)),
    ((10, 3, 3, 3, True, 2, 4, 16, 8, 0), (1,)),
    ((10, 3, 3, 1, False, 0, 8, 1, 0, 1), (None,)),
    ((10, 3, 4, 1, True, 2, 0, 1, 0, 0), (0,)),
    ((10, 3, 4, 3, False, 0, 4, 1, 0, 1), (None,)),
    ((10, 3, 4, 1, False, 0, 8, 16, 0, 0), (1, 0)),
    ((10, 3, 8, 3, True, 0, 4, 1, 0, 0), (1,)),
    ((10, 3, 8, 1, False, 2, 8, 1, 0, 0), (0,)),
]


def test_every_setting_appears():
    col = list(zip(*[s for s, _ in CASES]))
    assert set(zip(col[0], col[1])) == {(2, 1), (4, 2), (10, 3)} and set(col[2]) == {1, 3, 4, 8}
    assert set(zip(col[3], col[4])) == {(1, False), (1, True), (3, False), (3, True)} and set(col[5]) == {0, 2} and set(col[6]) == {0, 4, 8}
    assert set(col[7]) == {1, 16} and set(col[8]) == {0, 8} and set(col[9]) == {0, 1}
    assert {lv for _, levels in CASES for lv in levels} == {None, 0, 1}
    for lb in (1, 3, 4, 8):                                  # every leaf width with both hashes and at every size
        assert {s[9] for s, _ in CASES if s[2] == lb} == {0, 1} and {s[0] for s, _ in CASES if s[2] == lb} == {2, 4, 10}


@pytest.mark.parametrize("s,levels", CASES, ids=lambda v: "-".join(str(int(x)) if x is not None else "d" for x in v))
def test_rows_proof_is_the_model(zk, orc, s, levels):
    lib = zk.load()
    log_n, log_b, lb, K, coset, D, c, q, g, h = s
    ref = rows_ref.proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, g)
    out = np.zeros(32 << 8, dtype=np.uint8)
    with zk.BatchContext(log_n, log_b, lb, hash=HASH_NAMES[h], queries=q, grind_bits=g, fold_log=K, coset_leaves=coset, stop_log=D, cap_log=c,
                         shared_rows=True) as bc:
        assert bc.shared_rows and lib.zk_batch_get_shared_rows(bc._h) == 1
        bc.gen_fibsq(*_seeds(1 << lb))
        for on in levels:
            if on is not None:
                assert lib.zk_batch_set_host_levels(bc._h, on) == 0
            _same(bc.prove_shared(), ref, lib, s)
        # tree 0 is the tree over the rows, not the batch's heap: not reported
        assert lib.zk_batch_merkle_nodes(bc._h, 0, 0, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE
        assert lib.zk_batch_merkle_cap(bc._h, 0, 0, out.ctypes.data_as(C.c_void_p), out.size) == ERR_STATE
        assert lib.zk_batch_merkle_nodes(bc._h, 1, 0, 1, out.ctypes.data_as(C.c_void_p)) == ERR_STATE


def test_live_batch_alternates_all_three(zk, orc):
    """zk_batch_prove, shared without and with row leaves, twice round on one batch (the second round with K = 3, coset leaves and a cap):
    every output is its own model's, so tree 0 and the gather buffers are whole again after each call."""
    lib = zk.load()
    log_n, log_b, lb, q = 7, 2, 4, 2
    nb = 1 << lb
    out = np.zeros(32 << 8, dtype=np.uint8)
    optr = out.ctypes.data_as(C.c_void_p)

    def plain_ok(bc, K, coset, c):
        got = bc.prove()
        with zk.Context(log_n, log_b, queries=q, fold_log=K, coset_leaves=coset, cap_log=c) as ctx:
            for p in (0, 5, nb - 1):
                want = ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, SEED + p))
                assert got[p].data == want.data and got[p].state == want.state and got[p].public_last == want.public_last
        assert lib.zk_batch_merkle_cap(bc._h, 0, nb - 1, optr, out.size) == 0 and lib.zk_batch_merkle_cap(bc._h, 1, nb - 1, optr, out.size) == 0

    def shared_ok(bc, K, coset, c):
        bc.set_shared_rows(False)
        ref = shared_ref.proof(orc, log_n, log_b, lb, q, 0, K, coset, 0, c)
        got = bc.prove_shared()
        assert not got.shared_rows and got.data == ref.data and got.state == ref.state and got.check(strict=True) == 0
        for p in (0, nb - 1):                               # tree 0 is the batch's f heap again
            assert bc.merkle_cap(0, p).tobytes() == cap_ref.cap_of(ref.c.f_trees[p], ref.c.ce[0])

    def rows_ok(bc, K, coset, c):
        bc.set_shared_rows(True)
        _same(bc.prove_shared(), rows_ref.proof(orc, log_n, log_b, lb, q, 0, K, coset, 0, c), lib, (log_n, log_b, lb, K, coset, 0, c, q, 0, 0))
        assert lib.zk_batch_merkle_nodes(bc._h, 0, nb - 1, 1, optr) == ERR_STATE and lib.zk_batch_merkle_cap(bc._h, 0, 0, optr, out.size) == ERR_STATE

    with zk.BatchContext(log_n, log_b, lb, queries=q) as bc:
        bc.gen_fibsq(*_seeds(nb))
        before = bc.device_bytes
        for K, coset, c in ((1, False, 0), (3, True, 3)):
            bc.set_fold(K)
            bc.set_coset_leaves(coset)
            bc.set_merkle_cap(c)
            sized = bc.device_bytes
            plain_ok(bc, K, coset, c)
            shared_ok(bc, K, coset, c)
            rows_ok(bc, K, coset, c)
            rows_ok(bc, K, coset, c)
            assert bc.device_bytes == sized                 # neither kind of shared proof allocates on the device
        assert before <= bc.device_bytes
        plain_ok(bc, 3, True, 3)                            # zk_batch_prove does not look at the setting


def test_a_broken_trace_fails_the_batch_check(zk, orc):
    lib = zk.load()
    log_n, log_b, lb, q = 5, 2, 4, 1
    nb, n = 1 << lb, 1 << log_n
    good = np.stack([zk.trace_fibsq(n - 1, 1, SEED + p) for p in range(nb)]).astype(np.uint32)
    bad = good.copy()
    bad[9, 11] = (int(bad[9, 11]) + 1) % rows_ref.P
    for K, coset, D in ((1, False, 0), (3, True, 2)):
        with zk.BatchContext(log_n, log_b, lb, queries=q, fold_log=K, coset_leaves=coset, stop_log=D, shared_rows=True) as bc:
            bc.set_traces(bad)
            with pytest.raises(zk.ZkError) as e:
                bc.prove_shared()
            assert e.value.code == ERR_CHECK and "some trace of the batch" in str(e.value)
            bc.set_traces(good)
            _same(bc.prove_shared(), rows_ref.proof(orc, log_n, log_b, lb, q, 0, K, coset, D, 0), lib, (log_n, log_b, lb, K, coset, D, 0, q, 0, 0))


def test_refusals(zk, orc):
    lib = zk.load()
    state, got = np.zeros(32, dtype=np.uint8), C.c_size_t(0)
    buf = np.zeros(1 << 16, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for lb in (0, 9):                                        # as without row leaves: a batch of one is a plain proof, 2^9 are too many
        with zk.BatchContext(4, 1, lb, shared_rows=True) as bc:
            bc.gen_fibsq(*_seeds(1 << lb))
            assert lib.zk_batch_prove_shared(bc._h, ptr(buf), buf.size, C.byref(got), ptr(state)) == ERR_INVALID
            assert "log_batch" in lib.zk_last_error().decode()
    with zk.BatchContext(4, 1, 2) as bc:
        assert lib.zk_batch_get_shared_rows(bc._h) == 0      # off at creation
        assert lib.zk_batch_set_shared_rows(bc._h, 1) == 0 and lib.zk_batch_get_shared_rows(bc._h) == 1
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), buf.size, C.byref(got), ptr(state)) == ERR_STATE   # no traces
        bc.gen_fibsq(*_seeds(4))
        want = lib.zk_proof_data_len_shared_rows(4, 1, 1, 0, 1, 0, 0, 0, 2, 1)
        assert want < lib.zk_proof_data_len_shared(4, 1, 1, 0, 1, 0, 0, 0, 2)
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), want - 1, C.byref(got), ptr(state)) == ERR_BUFFER
        assert got.value == want and str(want) in lib.zk_last_error().decode()
        assert lib.zk_batch_prove_shared(bc._h, None, want, C.byref(got), ptr(state)) == ERR_INVALID
        assert lib.zk_batch_prove_shared(bc._h, ptr(buf), want, C.byref(got), ptr(state)) == 0
        assert buf[:want].tobytes() == rows_ref.proof(orc, 4, 1, 2, 1, 0, 1, False, 0, 0).data
    with pytest.raises(ValueError):
        zk.BatchContext(4, 1, 2, hash="blake2s", shared_rows=True)


def test_the_setter_is_refused_while_a_proof_runs(zk, orc):
    """prove_shared on one thread, zk_batch_set_shared_rows(on) on another: the setter is refused with ZK_ERR_STATE or succeeds between
    two proofs, and every proof is the model's."""
    lib = zk.load()
    log_n, log_b, lb = 10, 3, 3
    ref = rows_ref.proof(orc, log_n, log_b, lb, 1, 0, 1, False, 0, 0)
    with zk.BatchContext(log_n, log_b, lb, shared_rows=True) as bc:
        bc.gen_fibsq(*_seeds(1 << lb))
        proofs, errors = [], []

        def run():
            for _ in range(6):
                try:
                    proofs.append(bc.prove_shared())
                except zk.ZkError as e:                      # the setter held the batch
                    errors.append(e.code)

        t = threading.Thread(target=run)
        t.start()
        codes = []
        while t.is_alive() and len(codes) < 200:
            codes.append(lib.zk_batch_set_shared_rows(bc._h, 1))
        t.join()
        assert set(codes) <= {0, ERR_STATE} and set(errors) <= {ERR_STATE}, (codes, errors)
        for p in proofs:
            assert p.data == ref.data and p.state == ref.state
        assert proofs or errors
