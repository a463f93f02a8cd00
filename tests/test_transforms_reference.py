"""CPU pins of the references that tests/test_gpu_transforms.py checks the device against (tests/transforms_ref.py):
the arbitrary-shift, log_blowup >= 0 LDE must be orc.lde at the reference's shift 5 and the sharded test double's
definition at a shard shift 5 * h^r."""
import numpy as np
import pytest

import transforms_ref as ref

P = ref.P


def test_powers_and_mulmod():
    x = 3141592653 % P
    assert ref.powers(x, 1).tolist() == [1]
    assert ref.powers(x, 37).tolist() == [pow(x, k, P) for k in range(37)]
    a = np.array([0, 1, P - 1, P - 1, 2**31], dtype=np.uint32)
    b = np.array([P - 1, P - 1, P - 1, 2, 2**31], dtype=np.uint32)
    assert ref.mulmod(a, b).tolist() == [int(u) * int(v) % P for u, v in zip(a, b)]


def test_rand_field_is_canonical_uint32():
    v = ref.rand_field(np.random.default_rng(1), 3000, chunk=1024)
    assert v.dtype == np.uint32 and len(v) == 3000 and int(v.max()) < P and len(np.unique(v)) > 2900


@pytest.mark.parametrize("log_n,log_b", [(1, 1), (2, 0), (4, 3), (7, 5), (10, 0), (12, 4), (16, 2), (18, 0)])
def test_lde_reference_is_the_oracle_at_shift_5(orc, log_n, log_b):
    rng = np.random.default_rng(900 + 8 * log_n + log_b)
    trace = ref.rand_field(rng, (1 << log_n) - 1)
    trace[0] = P - 1
    assert np.array_equal(ref.lde_ref(orc, trace, log_n, log_b, 5), orc.lde(trace, log_n, log_b))


@pytest.mark.parametrize("log_n,log_b,rank_exp", [(2, 0, 1), (6, 0, 5), (7, 1, 3), (9, 2, 1), (10, 3, 6)])
def test_lde_reference_is_the_test_double_at_a_shard_shift(orc, log_n, log_b, rank_exp):
    from sharded_testlib import OracleBackend
    hglob = pow(5, (P - 1) >> (log_n + log_b + 3), P)
    shift = 5 * pow(hglob, rank_exp, P) % P
    assert shift != 5
    ob = OracleBackend()
    dom = ob.domain(log_n, log_b, shift)
    n, N = 1 << log_n, 1 << (log_n + log_b)
    trace = ref.rand_field(np.random.default_rng(950 + log_n), n - 1)
    out = ob.empty(N)
    ob.lde(dom, ob.upload(np.concatenate([trace, np.zeros(1, dtype=np.uint32)])), ob.empty(n), out)
    assert np.array_equal(ref.lde_ref(orc, trace, log_n, log_b, shift), ob.to_host(out))


@pytest.mark.parametrize("log_n", [2, 5, 12])
def test_linear_trace_lde_formula(orc, log_n):
    """The closed form that checks the 2^30-point LDE of a linear trace, against the transform reference."""
    c0, c1, n = 123456789, 2718281828, 1 << log_n
    t = ref.linear_trace(log_n, c0, c1, chunk=4)
    g = pow(5, (P - 1) >> log_n, P)
    assert t[:n - 1].tolist() == [(c0 + c1 * pow(g, i, P)) % P for i in range(n - 1)] and t[n - 1] == 0
    want = ref.lde_ref(orc, t[:n - 1], log_n, 0, 5)
    got = np.concatenate([ref.linear_lde_expected(t, log_n, c0, c1, 5, i, min(i + 8, n)) for i in range(0, n, 8)])
    assert np.array_equal(got, want)
