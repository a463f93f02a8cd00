"""The two kernels that run over E = F_P[u] / (u^2 - 5) (zk_dev_compose_ext, zk_dev_fri_fold_multi_ext) on the GPU.

compose: cp is linear in the alphas and the quotients stay in the base field, so plane j must be zk_dev_compose with the component-j
alphas word for word -- no model needed.  fold: against tests/ext_ref.py at the boundaries of the launch, which are the base-field
launch's (one lane; 2 outputs, the last narrow size; 4, the first wide one; 1024 = one full workgroup of the wide form; 2048 = two; 512
from a pointer one word past a 16-byte boundary = the narrow form across two workgroups), and with beta = (beta0, 0) against
zk_dev_fri_fold_multi of each plane."""
import ctypes as C

import numpy as np
import pytest

import ext_ref
from transforms_ref import P, rand_field

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A            # the words on either side of an output buffer must still hold this after a launch
PAD = 8                       # words: a multiple of 16 bytes, so the output keeps the alignment asked for


@pytest.fixture(scope="module")
def hb():
    from sharded_mirror import HipBackend
    b = HipBackend(0)
    yield b
    b.close()


def _out_buffer(hb, words, off):
    """`words` output words starting `off` words past a 16-byte boundary, with PAD guard words on either side."""
    lo = PAD + off
    whole = hb.empty(lo + words + PAD)
    whole.fill_(GUARD)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[lo:lo + words], lo


def _guards_intact(hb, whole, lo, words):
    host = hb.to_host(whole)
    return bool(np.all(host[:lo] == GUARD) and np.all(host[lo + words:] == GUARD))


def _in_buffer(hb, arr, off):
    buf = hb.empty(len(arr) + 4)
    src = buf[off:off + len(arr)]
    src.copy_(hb.upload(arr))
    assert src.data_ptr() % 16 == 4 * off
    return src


def _compose(hb, dom, f, first, last, alphas, off=0):
    from zkstark_amd._lib import check
    whole, cp, lo = _out_buffer(hb, len(f), off)
    a = (C.c_uint32 * 3)(*alphas)
    check(hb.lib.zk_dev_compose(dom, _in_buffer(hb, f, off).data_ptr(), cp.data_ptr(), first, last, a, hb._stream()))
    return hb.to_host(cp)


def _compose_ext(hb, dom, f, first, last, alphas6, off=0):
    from zkstark_amd._lib import check
    whole, cp, lo = _out_buffer(hb, 2 * len(f), off)
    a = (C.c_uint32 * 6)(*alphas6)
    check(hb.lib.zk_dev_compose_ext(dom, _in_buffer(hb, f, off).data_ptr(), cp.data_ptr(), first, last, a, hb._stream()))
    assert _guards_intact(hb, whole, lo, 2 * len(f))
    return hb.to_host(cp)


# logN = log_n + log_b: 3 is the narrow form, 4 the first wide one; log_b = 1, 2 take the window path of the wide form, 3 whole vectors
COMPOSE_SHAPES = [(2, 1), (3, 1), (2, 2), (2, 3), (12, 1), (11, 2), (10, 3)]


@pytest.mark.parametrize("log_n,log_b", COMPOSE_SHAPES)
def test_each_plane_of_compose_ext_is_compose_with_that_component(hb, log_n, log_b):
    N = 1 << (log_n + log_b)
    rng = np.random.default_rng(1000 * log_n + log_b)
    dom = hb.domain(log_n, log_b, 5)
    f = rand_field(rng, N)
    f[0], f[1], f[-1] = 0, P - 1, P - 1
    first, last = int(f[0]), int(rng.integers(0, P))
    alpha_sets = [[int(v) for v in rng.integers(0, P, 6)],
                  [P + 3, 2**32 - 1, 0, P - 1, 1, P],                      # raws >= P in both components; 0 and P (= 0) among them
                  [int(v) for v in rng.integers(0, 2**32, 3) for _ in (0, 1)]]
    alpha_sets[2][1::2] = [0, 0, 0]                                         # every component-1 raw zero
    for alphas in alpha_sets:
        for off in ((0, 1) if N > 8 else (0,)):                            # off = 1: the narrow form whatever the size
            got = _compose_ext(hb, dom, f, first, last, alphas, off)
            for j in (0, 1):
                want = _compose(hb, dom, f, first, last, alphas[j::2], off)
                assert np.array_equal(got[j * N:(j + 1) * N], want), (alphas, off, j)
    assert not got[N:].any()                                                # the last set: plane 1 all zero
    assert got[:N].any()


def _fold_ext(hb, dom, planes, log_m, rnd, steps, beta, off=0):
    from zkstark_amd._lib import check
    words = 2 * (len(planes) // 2 >> steps)
    whole, dst, lo = _out_buffer(hb, words, off)
    b = (C.c_uint32 * 2)(*beta)
    check(hb.lib.zk_dev_fri_fold_multi_ext(dom, _in_buffer(hb, planes, off).data_ptr(), dst.data_ptr(), log_m, rnd, steps, b, hb._stream()))
    assert _guards_intact(hb, whole, lo, words)
    return hb.to_host(dst)


def _fold_base(hb, dom, layer, log_m, rnd, steps, beta, off=0):
    from zkstark_amd._lib import check
    whole, dst, lo = _out_buffer(hb, len(layer) >> steps, off)
    check(hb.lib.zk_dev_fri_fold_multi(dom, _in_buffer(hb, layer, off).data_ptr(), dst.data_ptr(), log_m, rnd, steps, beta, hb._stream()))
    return hb.to_host(dst)


BETAS = [(P + 5, 2**32 - 1), (0, 123456789), (P - 1, P - 1), (1, 0), (0, 0)]        # raws >= P; (0, beta1); the extremes
FOLD_OUTPUTS = [(1, 0), (2, 0), (4, 0), (1024, 0), (2048, 0), (512, 1)]             # (outputs per call, words past a 16-byte boundary)


@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("q,off", FOLD_OUTPUTS)
def test_fold_ext_matches_the_model(hb, q, off, steps):
    lq = q.bit_length() - 1
    for rnd in (0, 3):
        log_m = lq + steps
        log_b = min(lq, 2)
        log_n = log_m + rnd - log_b                                          # rnd + steps <= log_n because log_b <= lq
        dom = hb.domain(log_n, log_b, ext_ref.SHIFT, fold_only=True)
        m = 1 << log_m
        rng = np.random.default_rng(100 * q + 10 * steps + rnd)
        planes = rand_field(rng, 2 * m)
        planes[0], planes[m] = 0, P - 1                                      # value 0 of E is (0, P - 1); the last is (P - 1, 0)
        planes[m - 1], planes[2 * m - 1] = P - 1, 0
        if m >= 4:
            planes[1], planes[m + 1] = 0, 0
            planes[2], planes[m + 2] = P - 1, P - 1
        for beta in BETAS + [tuple(int(v) for v in rng.integers(0, 2**32, 2))]:
            got = _fold_ext(hb, dom, planes, log_m, rnd, steps, beta, off)
            want = ext_ref.fold_layer(planes, log_n, log_b, rnd, steps, beta)
            assert np.array_equal(got, want), (rnd, beta)
        beta0 = int(rng.integers(0, 2**32))                                  # no model: beta = (beta0, 0) folds each plane by itself
        got = _fold_ext(hb, dom, planes, log_m, rnd, steps, (beta0, 0), off)
        for j in (0, 1):
            assert np.array_equal(got[j * q:(j + 1) * q], _fold_base(hb, dom, planes[j * m:(j + 1) * m], log_m, rnd, steps, beta0, off)), (rnd, j)


def test_fold_ext_refuses_what_the_base_fold_refuses(hb):
    lib = hb.lib
    dom = hb.domain(5, 3, 5, fold_only=True)
    a, b = hb.empty(2 << 8), hb.empty(2 << 8)
    beta = (C.c_uint32 * 2)(1, 2)
    for steps in (0, 4):
        assert lib.zk_dev_fri_fold_multi_ext(dom, a.data_ptr(), b.data_ptr(), 8, 0, steps, beta, hb._stream()) == -1
    assert lib.zk_dev_fri_fold_multi_ext(dom, a.data_ptr(), b.data_ptr(), 4, 4, 3, beta, hb._stream()) == -1     # round + steps beyond the rounds
    assert lib.zk_dev_fri_fold_multi_ext(dom, a.data_ptr(), b.data_ptr(), 7, 0, 2, beta, hb._stream()) == -1     # size does not match the round
    assert lib.zk_dev_fri_fold_multi_ext(dom, a.data_ptr(), b.data_ptr(), 8, 0, 2, None, hb._stream()) == -1
    assert lib.zk_dev_fri_fold_multi_ext(dom, a.data_ptr(), b.data_ptr(), 8, 0, 2, beta, hb._stream()) == 0
    dom2 = hb.domain(5, 3, 5, fold_only=True)
    six = (C.c_uint32 * 6)(1, 2, 3, 4, 5, 6)
    assert lib.zk_dev_compose_ext(dom2, a.data_ptr(), b.data_ptr(), 1, 2, six, hb._stream()) == -4                # a fold-only domain
    hb.sync()
