"""The batched verifier's shared-proof kernels as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): every instance exists and
uses no scratch, no LDS, no AGPRs and at most 128 VGPRs (csrc/verify.hip promises it; the row leaf streams its blocks through registers and
the layout table is indexed at run time, neither of which may have become a private array), and the kernels of plain proofs are still
there under their names."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHARED_KERNELS = ([f"verify_shared_algebra_kernel<{c}, {r}>" for c in ("false", "true") for r in ("false", "true")]
                  + [f"verify_shared_f_paths_kernel<{h}>" for h in (0, 1)]
                  + [f"verify_shared_row_paths_kernel<{h}>" for h in (0, 1)]
                  + [f"verify_shared_paths_kernel<{h}, {c}>" for h in (0, 1) for c in ("false", "true")]
                  + [f"verify_shared_transcript_kernel<{c}>" for c in ("false", "true")])
PLAIN_KERNELS = (["verify_algebra_kernel<false>", "verify_algebra_kernel<true>", "verify_transcript_kernel<false>", "verify_transcript_kernel<true>"]
                 + [f"verify_paths_kernel<{h}, {c}>" for h in (0, 1) for c in ("false", "true")])


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


def _one(rows, want):
    hit = [r for r in rows if r["demangled"].endswith("::" + want) or ("::" + want + "(") in r["demangled"]]
    assert len(hit) == 1, (want, [r["demangled"] for r in rows if "verify" in r["demangled"]])
    return hit[0]


@pytest.mark.parametrize("name", SHARED_KERNELS)
def test_shared_kernels_exist_within_their_budget(rows, name):
    r = _one(rows, name)
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= 128, r                    # four waves per SIMD at least


def test_plain_kernels_keep_their_names(rows):
    for name in PLAIN_KERNELS:
        r = _one(rows, name)
        assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
        assert r["vgpr"] <= 128, r
