"""The batched verifier's Merkle-cap kernels as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): the new kernels exist and
use neither scratch nor LDS (csrc/verify.hip promises both; their per-tree layout table is indexed at run time, which must not have
become a private copy), and the kernels of cap 0 are still there under their names."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAP_KERNELS = ["verify_cap_algebra_kernel<false>", "verify_cap_algebra_kernel<true>",
               "verify_cap_paths_kernel<0, false>", "verify_cap_paths_kernel<0, true>", "verify_cap_paths_kernel<1, false>", "verify_cap_paths_kernel<1, true>",
               "verify_cap_transcript_kernel<false>", "verify_cap_transcript_kernel<true>"]
CAP0_KERNELS = (["verify_algebra_kernel", "verify_stop_algebra_kernel", "verify_coset_paths_kernel<0>", "verify_coset_paths_kernel<1>"]
                + [f"verify_paths_kernel<{h}, {f}>" for h in (0, 1) for f in ("false", "true")]
                + [f"verify_fold_algebra_kernel<{k}, {s}>" for k in (2, 3) for s in ("false", "true")]
                + [f"verify_coset_algebra_kernel<{k}, {s}>" for k in (1, 2, 3) for s in ("false", "true")]
                + [f"verify_transcript_kernel<{a}>" for a in ("false, false, false", "false, false, true", "true, false, false", "true, false, true",
                                                               "true, true, false", "true, true, true")])


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


@pytest.mark.parametrize("name", CAP_KERNELS)
def test_cap_kernels_exist_without_scratch_or_lds(rows, name):
    r = _one(rows, name)
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= 128, r                    # four waves per SIMD at least, as the widest kernel of cap 0 (the field-hash paths: 88)


def test_cap0_kernels_keep_their_names(rows):
    for name in CAP0_KERNELS:
        r = _one(rows, name)
        assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0, r
