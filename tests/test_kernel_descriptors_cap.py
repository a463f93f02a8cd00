"""The batched verifier's plain-proof kernels as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): the three kernels that read
the layout table exist, one instance per leaf format and hash, and use neither scratch nor LDS (csrc/verify.hip promises both; the per-tree
table is indexed at run time, which must not have become a private copy); and the closed-form kernels they replaced at cap 0 are gone."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ["verify_algebra_kernel<false>", "verify_algebra_kernel<true>",
           "verify_paths_kernel<0, false>", "verify_paths_kernel<0, true>", "verify_paths_kernel<1, false>", "verify_paths_kernel<1, true>",
           "verify_transcript_kernel<false>", "verify_transcript_kernel<true>"]
# the 24 instances that computed the offsets of a cap-0 proof in closed form
REMOVED_KERNELS = (["verify_algebra_kernel", "verify_stop_algebra_kernel", "verify_coset_paths_kernel<0>", "verify_coset_paths_kernel<1>"]
                   + [f"verify_paths_kernel<{h}, {f}>" for h in (0, 1) for f in ("false", "true")]
                   + [f"verify_fold_algebra_kernel<{k}, {s}>" for k in (2, 3) for s in ("false", "true")]
                   + [f"verify_coset_algebra_kernel<{k}, {s}>" for k in (1, 2, 3) for s in ("false", "true")]
                   + [f"verify_transcript_kernel<{a}>" for a in ("false, false, false", "false, false, true", "true, false, false", "true, false, true",
                                                                  "true, true, false", "true, true, true")])
# of those, the names that the kernels of today carry as well: verify_paths_kernel<HASH, COSET> was <HASH, FOLD>
REUSED_NAMES = [f"verify_paths_kernel<{h}, {f}>" for h in (0, 1) for f in ("false", "true")]


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


def _hits(rows, want):
    return [r for r in rows if r["demangled"].endswith("::" + want) or ("::" + want + "(") in r["demangled"]]


def _one(rows, want):
    hit = _hits(rows, want)
    assert len(hit) == 1, (want, [r["demangled"] for r in rows if "verify" in r["demangled"]])
    return hit[0]


@pytest.mark.parametrize("name", KERNELS)
def test_cap_kernels_exist_without_scratch_or_lds(rows, name):
    r = _one(rows, name)
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= 128, r                    # four waves per SIMD at least (the widest, the field-hash paths: 88)


def test_closed_form_kernels_are_gone(rows):
    assert len(REMOVED_KERNELS) == 24
    for name in REMOVED_KERNELS:
        if name not in REUSED_NAMES:
            assert _hits(rows, name) == [], name
    for stem in ("verify_stop_algebra", "verify_fold_algebra", "verify_coset_algebra", "verify_coset_paths", "verify_cap_"):
        assert [r["demangled"] for r in rows if stem in r["demangled"]] == [], stem
