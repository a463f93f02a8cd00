"""The batched GPU verifier on stopped proofs made by the one-call prover (Context(stop_log=D) -> Verifier(stop_log=D)): the GPU's
check numbers are 0 and equal zk_verify_stop's, and a proof with one coefficient byte flipped is rejected with the CPU's number.
This is the only verifier test that runs the prover's early-stop path (fri_final_poly_kernel); tests/test_gpu_verify_stop.py needs
no prover at all."""
import ctypes as C

import numpy as np
import pytest

import stop_ref

pytestmark = pytest.mark.gpu


def _cpu(lib, data, state, log_n, log_b, last, K, coset, D):
    c = C.c_int32(12345)
    lib.zk_verify_stop(data, len(data), state, log_n, log_b, last, 0, 1, 0, K, int(coset), D, C.byref(c))
    return c.value


@pytest.mark.parametrize("coset", [False, True], ids=["plain", "coset"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("log_n,log_b", [(6, 3), (10, 3)])
def test_prover_proofs_pass_the_batched_verifier(zk, log_n, log_b, K, coset):
    lib = zk.load()
    largest = max(D for D in range(1, 9) if stop_ref.admissible(log_n, log_b, D))
    for D in sorted({2, largest}):
        with zk.Context(log_n, log_b, fold_log=K, coset_leaves=coset, stop_log=D) as ctx:
            proofs = [ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, 3141592 + i)) for i in range(3)]
        assert all(p.stop_log == D and len(p.data) == p.expected_len() for p in proofs)
        # one coefficient byte flipped in a copy of proof 0: coefficient 2^D - 1, the last word before the query raw
        G = len(stop_ref.groups(log_n - D, K))
        off = 76 + 36 * (G - 1) + 4 + 4 * ((1 << D) - 1)
        bad = bytearray(proofs[0].data)
        bad[off] ^= 0x04
        rows = [(p.data, p.state, p.public_last & 0xFFFFFFFF) for p in proofs] + [(bytes(bad), proofs[0].state, proofs[0].public_last & 0xFFFFFFFF)]
        with zk.Verifier(log_n, log_b, fold_log=K, coset_leaves=coset, stop_log=D) as v:
            assert v.proof_len == len(proofs[0].data)
            assert (v.verify(proofs) == 0).all()
            data = np.stack([np.frombuffer(d, dtype=np.uint8) for d, _, _ in rows])
            states = np.stack([np.frombuffer(s, dtype=np.uint8) for _, s, _ in rows])
            for strict in (True, False):
                want = np.array([_cpu(lib, d, s if strict else None, log_n, log_b, last, K, coset, D) for d, s, last in rows], dtype=np.int32)
                got = v.verify_raw(data, [last for _, _, last in rows], states if strict else None)
                assert np.array_equal(got, want), (D, strict, got, want)
                assert (want[:3] == 0).all() and want[3] != 0, (D, strict, want)
                if not strict:
                    assert want[3] == -(100 + (G - 1))
