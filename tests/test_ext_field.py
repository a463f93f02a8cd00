"""E = F_P[u] / (u^2 - 5) on the host (zk_ext_mul / zk_ext_inv / zk_ext_pow, zkstark_amd.ext_*) against Python
integers (tests/ext_ref.py), and the model's fold against the oracle's base-field fold where the two must agree."""
import ctypes as C
import random

import numpy as np
import pytest

import ext_ref
from ext_ref import P

ERR_INVALID = -1
EDGES = [(0, 0), (P - 1, P - 1), (0, 1), (1, 0), (P - 1, 0), (0, P - 1), (5, 0), (1, 1)]


def _pairs(seed, count):
    rng = random.Random(seed)
    return EDGES + [(rng.randrange(P), rng.randrange(P)) for _ in range(count)]


def test_five_is_a_non_residue():
    assert pow(5, (P - 1) // 2, P) == P - 1


def test_mul_matches_python_integers(zk):
    pairs = _pairs(1, 40)
    for a in pairs:
        for b in pairs:
            assert zk.ext_mul(a, b) == ext_ref.mul(a, b), (a, b)
    assert zk.ext_mul((0, 1), (0, 1)) == (5, 0)
    assert zk.ext_mul((P - 1, P - 1), (P - 1, P - 1)) == ((1 + 5) % P, 2)            # (-1 - u)^2 = 1 + 5 + 2 u


def test_raws_above_p_are_reduced(zk):
    for a, b in [((P, P + 1), (2**32 - 1, P + 7)), ((2**32 - 1, 2**32 - 1), (2**32 - 1, 2**32 - 1))]:
        assert zk.ext_mul(a, b) == ext_ref.mul(a, b)
        assert zk.ext_pow(a, 3) == ext_ref.power(a, 3)
    assert zk.ext_inv((P + 2, P)) == ext_ref.inv((2, 0))


def test_inverse(zk):
    for a in _pairs(2, 200):
        if a == (0, 0):
            continue
        ai = zk.ext_inv(a)
        assert ai == ext_ref.inv(a), a
        assert zk.ext_mul(a, ai) == (1, 0), a


def test_the_inverse_of_zero_is_refused(zk):
    lib = zk.load()
    out = (C.c_uint32 * 2)(7, 7)
    for zero in ((0, 0), (P, P), (0, P)):
        assert lib.zk_ext_inv((C.c_uint32 * 2)(*zero), out) == ERR_INVALID
        assert b"zero" in lib.zk_last_error()
        assert tuple(out) == (7, 7)
    with pytest.raises(ZeroDivisionError):
        zk.ext_inv((0, 0))


def test_pow(zk):
    rng = random.Random(3)
    for a in _pairs(3, 20):
        for e in (0, 1, 2, 3, P - 1, P, P + 1, P * P - 2, P * P - 1, rng.randrange(2**64), 2**64 - 1):
            assert zk.ext_pow(a, e) == ext_ref.power(a, e), (a, e)
        if a != (0, 0):
            assert zk.ext_pow(a, P * P - 1) == (1, 0)                                  # the order of E* is P^2 - 1
            assert zk.ext_pow(a, P * P - 2) == zk.ext_inv(a)
    assert zk.ext_pow((0, 1), P) == (0, P - 1)                                         # Frobenius: u^P = -u


def test_null_arguments_are_refused(zk):
    lib = zk.load()
    a, out = (C.c_uint32 * 2)(1, 2), (C.c_uint32 * 2)()
    assert lib.zk_ext_mul(None, a, out) == ERR_INVALID and lib.zk_ext_mul(a, None, out) == ERR_INVALID and lib.zk_ext_mul(a, a, None) == ERR_INVALID
    assert lib.zk_ext_inv(None, out) == ERR_INVALID and lib.zk_ext_inv(a, None) == ERR_INVALID
    assert lib.zk_ext_pow(None, 2, out) == ERR_INVALID and lib.zk_ext_pow(a, 2, None) == ERR_INVALID
    assert lib.zk_dev_compose_ext(None, None, None, 0, 0, None, None) == ERR_INVALID
    assert lib.zk_dev_fri_fold_multi_ext(None, None, None, 4, 0, 2, None, None) == ERR_INVALID


def test_out_may_alias_an_input(zk):
    lib = zk.load()
    a, b = (C.c_uint32 * 2)(3, P - 4), (C.c_uint32 * 2)(P - 1, 9)
    want = ext_ref.mul(tuple(a), tuple(b))
    assert lib.zk_ext_mul(a, b, a) == 0 and tuple(a) == want


@pytest.mark.parametrize("log_n,log_b", [(3, 1), (5, 2), (8, 3)])
def test_model_fold_with_a_base_field_challenge_is_the_oracle_fold_of_each_plane(orc, log_n, log_b):
    """With beta = (beta0, 0) the fold over E does not mix the planes: each is the oracle's fold of that plane with beta0, at every
    round -- which pins the model's points x_i, its halving and its plane layout to the oracle's."""
    rng = np.random.default_rng(log_n)
    for rnd in range(log_n):
        m = 1 << (log_n + log_b - rnd)
        planes = rng.integers(0, P, 2 * m, dtype=np.uint64).astype(np.uint32)
        planes[0], planes[m], planes[m - 1], planes[2 * m - 1] = 0, P - 1, P - 1, 0
        beta0 = int(rng.integers(0, P))
        got = ext_ref.fold_once(planes, log_n, log_b, rnd, (beta0, 0))
        for j in (0, 1):
            want = orc.fri_fold_eval(planes[j * m:(j + 1) * m], log_n, log_b, rnd, beta0)
            assert np.array_equal(got[j * (m // 2):(j + 1) * (m // 2)], want), (rnd, j)


def test_model_fold_halves_a_polynomial_with_coefficients_in_e():
    """The definition the fold stands for: on the evaluations of v(X) = sum c_k X^k, c_k in E, the fold with beta gives the evaluations of
    sum (c_2k + beta c_2k+1) Y^k at Y = x^2 -- with the product beta c taken in E."""
    log_n, log_b = 3, 1
    L = log_n + log_b
    rng = random.Random(11)
    h = pow(ext_ref.GEN_W, (P - 1) >> L, P)
    coef = [(rng.randrange(P), rng.randrange(P)) for _ in range(1 << log_n)]

    def evaluate(cs, x):
        acc = (0, 0)
        for c in reversed(cs):
            acc = ((acc[0] * x + c[0]) % P, (acc[1] * x + c[1]) % P)
        return acc

    for rnd in range(log_n):
        m = 1 << (L - rnd)
        xs = [pow(ext_ref.SHIFT * pow(h, i, P) % P, 1 << rnd, P) for i in range(m)]
        vals = [evaluate(coef, x) for x in xs]
        planes = np.array([v[0] for v in vals] + [v[1] for v in vals], dtype=np.uint32)
        beta = (rng.randrange(P), rng.randrange(1, P))
        got = ext_ref.fold_once(planes, log_n, log_b, rnd, beta)
        coef = [tuple((a + b) % P for a, b in zip(coef[2 * k], ext_ref.mul(beta, coef[2 * k + 1]))) for k in range(len(coef) // 2)]
        want = [evaluate(coef, x * x % P) for x in xs[:m // 2]]
        assert [(int(got[i]), int(got[m // 2 + i])) for i in range(m // 2)] == want, rnd
