"""The batched verifier's kernels for proofs over E as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): every instance
exists under its name and uses no scratch, no LDS, no AGPRs and at most 128 VGPRs, four waves per SIMD (csrc/verify.hip promises it: the
sixteen values of a full K = 3 group fold in registers with static indices, and the 16-word leaf streams through the chain of the row
leaf).  The measured counts are in DESIGN.md 7k; the kernels of ext-off verifiers are held by the descriptor tests they already have."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXT_KERNELS = ([f"verify_ext_algebra_kernel<{c}>" for c in ("false", "true")]
               + [f"verify_ext_paths_kernel<{h}, {c}>" for h in (0, 1) for c in ("false", "true")]
               + [f"verify_ext_transcript_kernel<{c}>" for c in ("false", "true")])


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_descriptors", os.path.join(ROOT, "tools", "kernel_descriptors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(os.path.join(mod.LLVM, "llvm-readelf")):
        pytest.skip("llvm tools not present")
    from zkstark_amd import _lib
    _lib.load()                                   # builds the library if needed
    return mod.collect()


@pytest.mark.parametrize("name", EXT_KERNELS)
def test_ext_kernels_exist_within_their_budget(rows, name):
    hit = [r for r in rows if r["demangled"].endswith("::" + name) or ("::" + name + "(") in r["demangled"]]
    assert len(hit) == 1, (name, [r["demangled"] for r in rows if "verify_ext" in r["demangled"]])
    r = hit[0]
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= 128, r                    # four waves per SIMD at least
