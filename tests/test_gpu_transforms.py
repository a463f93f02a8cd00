"""The transforms against the CPU oracle (bit-exact), every size up to 2^26 and chosen large shapes up to domain 2^30.

make_plan (csrc/domain.hip, kMaxRadixLog = 8) splits a size-2^k transform into radix passes:

    k       23      24      25       26       27       28       29       30
    digits  8,8,7   8,8,8   7,6,6,6  7,7,6,6  7,7,7,6  7,7,7,7  8,7,7,7  8,8,7,7

zk.ntt runs the plan of log_m; the LDE runs the plan of log_n on the size-2^(log_n + log_b) domain, its first pass
(the last digit) reading the n coefficients.  The small and medium shapes are swept exhaustively; the large domains,
which reach the four-pass plans and indexing near 2^32 bytes, go one test per shape through the domain API
(zk_dom_create + zk_dev_*), which needs a few words per point instead of a whole prover context.  Large cases skip,
saying why, when the device or the host has too little free memory (tests/transforms_ref.py require_memory).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import transforms_ref as ref
from transforms_ref import P, rand_field, require_memory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GiB = 1 << 30


def _edged(x):
    x[0] = P - 1
    x[-1] = P - 1
    return x


@pytest.fixture
def hb():
    from sharded_mirror import HipBackend
    b = HipBackend(0)
    yield b
    b.close()


def _dom_lde(hb, log_n, log_b, shift, trace):
    """zk_dev_lde on a fresh domain; returns (domain, device f)."""
    n = 1 << log_n
    dom = hb.domain(log_n, log_b, shift)
    t = hb.empty(n)
    t[:n - 1].copy_(hb.upload(trace))
    t[n - 1:].zero_()
    out = hb.empty(n << log_b)
    coef = hb.empty(2 * n)
    hb.lde(dom, t, coef, out)
    hb.sync()
    del t, coef
    return dom, out


# ---- 1. exhaustive small and medium shapes ------------------------------------------------------------------------
@pytest.mark.parametrize("log_m", range(1, 27))
def test_ntt_every_size_matches_oracle(zk, orc, log_m):
    """Forward and inverse zk.ntt at every size up to 2^26 (1 to 4 passes; 25, 26: the four-pass plans), random
    canonical input with P - 1 at both ends; from 2^23 on also the all-(P - 1) vector."""
    m = 1 << log_m
    if log_m >= 23:
        require_memory(4 * m * 4, 8 * m * 4)
    root = orc.gen_of_order_log(log_m)
    vecs = [_edged(rand_field(np.random.default_rng(2000 + log_m), m))]
    if log_m >= 23:
        vecs.append(np.full(m, P - 1, dtype=np.uint32))
    for x in vecs:
        assert np.array_equal(zk.ntt(x), orc.ntt(x, root)), "forward"
        assert np.array_equal(zk.ntt(x, inverse=True), orc.intt(x, root)), "inverse"


def test_ntt_refuses_non_power_of_two(zk):
    for m in (1, 3, 6):
        with pytest.raises(zk.ZkError):
            zk.ntt(np.ones(m, dtype=np.uint32))


def _ctx_accepts(log_n, log_b):
    # check_proof_size (csrc/internal.hpp): 2 <= log_n, 1 <= log_b <= 5, L <= 30, n = 8 refused
    return log_n >= 2 and log_n != 3 and 1 <= log_b <= 5


@pytest.mark.parametrize("log_n,log_b", [(ln, lb) for ln in range(1, 23) for lb in range(0, 7) if ln + lb <= 22])
def test_lde_every_context_shape_matches_oracle(zk, orc, log_n, log_b):
    """zk.lde (a zk_ctx) at every (log_n, log_b) with L <= 22 against orc.lde; the shapes zk_ctx_create refuses
    (log_b 0 or 6, n = 2 or 8) raise ZkError."""
    rng = np.random.default_rng(3000 + 8 * log_n + log_b)
    trace = _edged(rand_field(rng, (1 << log_n) - 1))
    if not _ctx_accepts(log_n, log_b):
        with pytest.raises(zk.ZkError):
            zk.lde(trace, log_n, log_b)
        return
    assert np.array_equal(zk.lde(trace, log_n, log_b), orc.lde(trace, log_n, log_b))


@pytest.mark.parametrize("log_n", range(1, 21))
def test_domain_lde_without_blowup(orc, hb, log_n):
    """zk_dev_lde with log_blowup = 0 (N = n: the first LDE pass reads one coefficient per column) at shift 5."""
    trace = _edged(rand_field(np.random.default_rng(4000 + log_n), (1 << log_n) - 1))
    _, out = _dom_lde(hb, log_n, 0, 5, trace)
    assert np.array_equal(hb.to_host(out), ref.lde_ref(orc, trace, log_n, 0, 5))


def _shard_shift(log_L, r):
    return 5 * pow(pow(5, (P - 1) >> (log_L + 3), P), r, P) % P


@pytest.mark.parametrize("log_n,log_b", [(16, 3), (10, 2), (20, 0), (12, 5), (2, 1)])
@pytest.mark.parametrize("shift", [2, 3, 7, P - 2, "shard"])
def test_domain_lde_other_shifts(orc, hb, log_n, log_b, shift):
    """zk_dev_lde on cosets other than 5 * <h> (the W table of shift powers, the coefficient preparation) against the
    plain reference; "shard" is 5 * h'^3 for h' of order 8N, a coset the sharded prover uses."""
    if shift == "shard":
        shift = _shard_shift(log_n + log_b, 3)
    trace = _edged(rand_field(np.random.default_rng(5000 + 8 * log_n + log_b + shift % 97), (1 << log_n) - 1))
    _, out = _dom_lde(hb, log_n, log_b, shift, trace)
    assert np.array_equal(hb.to_host(out), ref.lde_ref(orc, trace, log_n, log_b, shift))


def test_domain_refuses_shifts_in_the_subgroup(zk, hb):
    """x - 1 must be invertible on the domain: a shift with shift^N = 1 (h itself, a power of it, P - 1, and 3, whose
    order is 2^27, on a 2^27 domain) is refused, and so are 0 and non-canonical values."""
    for log_n, log_b in ((10, 3), (16, 0), (24, 3)):
        L = log_n + log_b
        h = pow(5, (P - 1) >> L, P)
        bad = [h, pow(h, 5, P), P - 1, 1, 0, P, 2**32 - 1] + ([3] if L >= 27 else [])
        for s in bad:
            with pytest.raises(zk.ZkError):
                hb.domain(log_n, log_b, s)
    hb.domain(10, 3, 3)                       # 3^N != 1 below 2^27: accepted


def _compose_fold_case(hb, log_n, log_b, shift, aligned, rounds, want_compose, want_fold):
    """zk_dev_compose then `rounds` zk_dev_fri_fold rounds.  aligned=False passes every buffer one word past a 16-byte
    boundary (a [1:] slice), which sends the launches to the scalar compose_kernel / fri_fold_kernel."""
    L = log_n + log_b
    N, off = 1 << L, 0 if aligned else 1
    rng = np.random.default_rng(6000 + 8 * log_n + log_b + off)
    f = _edged(rand_field(rng, N))
    last = int(rng.integers(0, P))
    alphas = [int(rng.integers(0, 2**32)), 3235878091, P]          # raw challenges >= P are reduced (field.rs:20-24)
    dom = hb.domain(log_n, log_b, shift)

    def buf(words):
        return hb.empty(words + off)[off:]

    fd, cd = buf(N), buf(N)
    assert (fd.data_ptr() % 16 == 0) == aligned
    fd.copy_(hb.upload(f))
    hb.compose(dom, fd, cd, 1, last, alphas)
    cp = hb.to_host(cd)
    assert np.array_equal(cp, want_compose(f, last, alphas)), "compose"
    layer_d, layer = cd, cp
    for r in range(rounds):
        beta = [int(rng.integers(0, 2**32)), P + 1, 2**32 - 1, 0][r % 4]
        nd = buf(N >> (r + 1))
        hb.fold(dom, layer_d, nd, L - r, r, beta)
        nxt = hb.to_host(nd)
        assert np.array_equal(nxt, want_fold(layer, r, beta)), f"fold round {r}"
        layer_d, layer = nd, nxt


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "scalar"])
def test_compose_and_fold_2e16_both_kernels(orc, hb, aligned):
    """Composition and every FRI round at domain 2^16 (shift 5) on compose_kernel4 / fri_fold_kernel4 and on the
    scalar kernels, which run at real sizes only when a buffer is not 16-byte aligned."""
    log_n, log_b = 13, 3
    _compose_fold_case(hb, log_n, log_b, 5, aligned, log_n,
                       lambda f, last, al: orc.compose(f, log_n, log_b, al, last),
                       lambda e, r, beta: orc.fri_fold_eval(e, log_n, log_b, r, beta))


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "scalar"])
def test_compose_and_fold_other_shift_both_kernels(hb, aligned):
    """As above on the coset 7 * <h> (2^12 points) against the definitions in the sharded test double."""
    from sharded_testlib import OracleBackend
    log_n, log_b, shift = 9, 3, 7
    ob = OracleBackend()
    do = ob.domain(log_n, log_b, shift)

    def want_compose(f, last, alphas):
        out = ob.empty(len(f))
        ob.compose(do, ob.upload(f), out, 1, last, alphas)
        return ob.to_host(out)

    def want_fold(e, r, beta):
        out = ob.empty(len(e) // 2)
        ob.fold(do, ob.upload(e), out, log_n + log_b - r, r, beta)
        return ob.to_host(out)

    _compose_fold_case(hb, log_n, log_b, shift, aligned, 5, want_compose, want_fold)


# ---- 2. large domains, one test per shape ---------------------------------------------------------------------------
def test_ntt_2e28_matches_oracle(zk, orc):
    """zk.ntt at 2^28, forward and inverse: plan 7,7,7,7, every pass radix 128."""
    m = 1 << 28
    require_memory(3 * m * 4, 7 * m * 4)
    x = _edged(rand_field(np.random.default_rng(28), m))
    root = orc.gen_of_order_log(28)
    got = zk.ntt(x)
    assert np.array_equal(got, orc.ntt(x, root)), "forward"
    del got
    got = zk.ntt(x, inverse=True)
    assert np.array_equal(got, orc.intt(x, root)), "inverse"


def test_ntt_2e30_matches_oracle(zk, orc):
    """zk.ntt at 2^30, the largest size: plan 8,8,7,7, the outermost pass spanning the whole 4 GiB buffer.  Forward
    against the oracle; the inverse by the round trip on the device."""
    m = 1 << 30
    require_memory(3 * m * 4, 6 * m * 4)
    x = _edged(rand_field(np.random.default_rng(30), m))
    got = zk.ntt(x)
    want = orc.ntt(x, orc.gen_of_order_log(30))
    assert np.array_equal(got, want), "forward"
    del want
    back = zk.ntt(got, inverse=True)
    del got
    assert np.array_equal(back, x), "inverse round trip"


def _large_lde(orc, hb, log_n, log_b, seed):
    n, N = 1 << log_n, 1 << (log_n + log_b)
    require_memory((3 * n + 2 * N) * 4 + GiB, (n + 3 * N) * 4)
    trace = _edged(rand_field(np.random.default_rng(seed), n - 1))
    dom, out = _dom_lde(hb, log_n, log_b, 5, trace)
    got = hb.to_host(out)
    del out
    assert np.array_equal(got, orc.lde(trace, log_n, log_b))


def test_lde_22_3_matches_oracle(orc, hb):
    """LDE (22, 3), domain 2^25: plan of 22 = 8,7,7 on the size-2^25 transform (first pass radix 128 over S = 8)."""
    _large_lde(orc, hb, 22, 3, 7223)


def test_lde_25_1_matches_oracle(orc, hb):
    """LDE (25, 1), domain 2^26: the four-pass plan 7,6,6,6, blow-up 2 (first pass over S = 2)."""
    _large_lde(orc, hb, 25, 1, 7251)


def test_lde_24_4_matches_oracle(orc, hb):
    """LDE (24, 4), domain 2^28: plan 8,8,8 with last digit 8, so the first pass has logC = 12 - 8 = log_b and
    ntt_fast_ok refuses it: the generic ntt_pass_kernel plus the separate coef_prepare sweep, on 2^28 words."""
    _large_lde(orc, hb, 24, 4, 7244)


def test_lde_compose_fold_27_3_matches_oracle(orc, hb):
    """LDE (27, 3), domain 2^30: plan 7,7,7,6 on the size-2^30 transform, four passes over a 4 GiB buffer; then
    zk_dev_compose and three zk_dev_fri_fold rounds from the same device buffers, each against the oracle."""
    log_n, log_b = 27, 3
    n, N, L = 1 << log_n, 1 << 30, 30
    require_memory((3 * n + 5 * N) * 4 + GiB, (n + 4 * N) * 4)
    rng = np.random.default_rng(7273)
    trace = _edged(rand_field(rng, n - 1))
    trace[0] = 1                                   # a[0]: orc.compose uses the literal 1 (proof.rs:69)
    dom, fd = _dom_lde(hb, log_n, log_b, 5, trace)
    f = hb.to_host(fd)
    assert np.array_equal(f, orc.lde(trace, log_n, log_b)), "lde"
    alphas = [int(rng.integers(0, 2**32)) for _ in range(3)]
    cd = hb.empty(N)
    hb.compose(dom, fd, cd, 1, int(trace[-1]), alphas)
    del fd
    cp = orc.compose(f, log_n, log_b, alphas, int(trace[-1]))
    del f
    assert np.array_equal(hb.to_host(cd), cp), "compose"
    layer_d, layer = cd, cp
    for r in range(3):
        beta = int(rng.integers(0, 2**32))
        nd = hb.empty(N >> (r + 1))
        hb.fold(dom, layer_d, nd, L - r, r, beta)
        want = orc.fri_fold_eval(layer, log_n, log_b, r, beta)
        del layer
        assert np.array_equal(hb.to_host(nd), want), f"fold round {r}"
        layer_d, layer = nd, want


def test_lde_30_0_end_of_buffer(hb):
    """LDE (30, 0), domain 2^30 with no blow-up (the domain API only): plan 8,8,7,7; the first pass (last digit 7,
    S = 1) reads the 2^30 coefficients one per column.  Through a buffer resource based at the array's start (record
    count 2^32 - 1) the last one sits at byte offset 2^32 - 4, which gfx950 reads as 0: this test failed so, with an
    error of exactly e * x^(n-1), before ntt_fast.hip based that resource per tile.  The trace is the linear
    polynomial q(x) = c0 + c1 x on <g>, so f_i = q(5 g^i) = c0 + 5 (t_i - c0) is exact without an oracle transform
    (tests/transforms_ref.py); a coefficient lost at the load changes every value."""
    log_n = 30
    n = 1 << log_n
    require_memory(5 * n * 4 + GiB, 4 * n * 4)
    c0, c1 = 123456789, 2718281828
    t = ref.linear_trace(log_n, c0, c1)
    dom = hb.domain(log_n, 0, 5)
    td, coef, out = hb.upload(t), hb.empty(2 * n), hb.empty(n)
    hb.lde(dom, td, coef, out)
    hb.sync()
    del td, coef
    got = hb.to_host(out)
    del out
    chunk = 1 << 24
    for i in range(0, n, chunk):
        want = ref.linear_lde_expected(t, log_n, c0, c1, 5, i, i + chunk)
        assert np.array_equal(got[i:i + chunk], want), f"values {i} .. {i + chunk - 1}"


def test_config4_golden_on_one_gpu(zk):
    """BASELINE configs[3] on one GPU with no oracle run: Context(23, 3) LDE (plan 8,8,7 on 2^26) and the Merkle
    commitment of f against tests/golden/config4_2e26.json (root, first 64 values, SHA-256 of the whole vector)."""
    with open(os.path.join(ROOT, "tests", "golden", "config4_2e26.json")) as fh:
        gold = json.load(fh)
    par, pin = gold["params"], gold["pinned"]
    log_n, log_b = par["log_n"], par["log_blowup"]
    require_memory(24 * 2**30, 2 * (1 << (log_n + log_b)) * 4)
    assert (par["a0"], par["a1"]) == (1, 3141592)
    trace = zk.trace_fibsq((1 << log_n) - 1)
    assert int(trace[-1]) == pin["trace_last"]
    with zk.Context(log_n, log_b) as ctx:
        ctx.trace_upload(trace)
        ctx.lde()
        root = ctx.merkle_commit(0)
        f = ctx.layer_read(0)
    assert len(f) == par["domain"]
    assert list(f[:64]) == pin["f_eval_head"]
    assert hashlib.sha256(np.ascontiguousarray(f, dtype="<u4").tobytes()).hexdigest() == pin["f_eval_sha256"]
    assert root.hex() == pin["f_eval_root"]
