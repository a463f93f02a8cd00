"""The batch form of the final-polynomial kernel in the built gfx950 code object (no GPU needed; tools/kernel_descriptors.py): it is
there, uses no scratch, and its LDS is the 24 KiB of values and twiddles plus one counter per layer of a workgroup."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_descriptors", os.path.join(ROOT, "tools", "kernel_descriptors.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    if not os.path.exists(os.path.join(kd.LLVM, "llvm-readelf")):
        pytest.skip("llvm tools not present")
    from zkstark_amd import _lib
    _lib.load()
    return kd.collect()


def test_batch_final_poly_kernel_is_built_without_scratch(rows):
    mine = [r for r in rows if "fri_final_poly_batch_kernel" in r["demangled"]]
    assert len(mine) == 1, [r["demangled"] for r in mine]
    r = mine[0]
    assert r["scratch"] == 0
    assert r["lds"] <= 24 * 1024 + 4 * 1024                 # x[4096] + tw[2048] words, and 1024 per-layer counters
    assert r["wg"] == 1024
    one = [r for r in rows if "fri_final_poly_kernel" in r["demangled"]]
    assert len(one) == 1 and one[0]["scratch"] == 0         # the one-proof kernel is still its own kernel
