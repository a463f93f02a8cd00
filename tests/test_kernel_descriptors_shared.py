"""The kernel of the shared proof (compose_sum_batch_kernel, csrc/kernels.hip: CP = the sum of a batch's composition polynomials) as built
for gfx950 (no GPU needed; tools/kernel_descriptors.py): it exists once, keeps its sums and the prefetched vectors in registers -- no
scratch, no LDS, no accumulation registers -- and its vector register count is recorded.  The Merkle, compose and fold kernels the
shared proof launches around it were not edited: they are still found under the names the other descriptor tests look for."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 3 x 4 sums, two sets of three 16-byte vectors (the current statement's and the next one's), 4 x (inv0, inv2, zz), addresses
VGPR_RECORDED = 64

KEPT = (["merkle_subtree_kernel<zk::PlainSrc, true, 0>", "merkle_subtree_kernel<zk::PlainSrc, false, 0>",
         "merkle_subtree_kernel<zk::PlainSrc, true, 1>", "merkle_subtree_kernel<zk::PlainSrc, false, 1>"]
        + [f"merkle_wg_kernel<zk::PlainSrc, {leaf}, {h}>" for leaf in ("true", "false") for h in (0, 1, 2)]
        + [f"merkle_subtree_kernel<zk::{src}, true, {h}>" for src in ("ComposeBatchSrc", "FoldBatchSrc") for h in (0, 1)]
        + [f"merkle_wg_kernel<zk::{src}, true, {h}>" for src in ("ComposeBatchSrc", "FoldBatchSrc") for h in (0, 1)]
        + [f"coset_leaf_hash_batch_kernel<{h}, {s}>" for h in (0, 1) for s in (1, 2, 3)]
        + ["compose_kernel", "compose_kernel4", "compose_batch_kernel", "digest_level_post_kernel"])


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


def _named(rows, want):
    return [r for r in rows if r["demangled"].endswith("::" + want) or ("::" + want + "(") in r["demangled"]]


def test_compose_sum_kernel_lives_in_registers(rows):
    hit = _named(rows, "compose_sum_batch_kernel")
    assert len(hit) == 1, [r["demangled"] for r in rows if "compose" in r["demangled"]]
    r = hit[0]
    print("compose_sum_batch_kernel:", r)
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0 and r.get("ds", 0) == 0, r
    assert r["vgpr"] <= VGPR_RECORDED, r


def test_neighbouring_kernels_keep_their_names(rows):
    for name in KEPT:
        assert len(_named(rows, name)) == 1, (name, sorted(r["demangled"] for r in rows if name.split("<")[0] in r["demangled"]))
    for want in ("merkle_subtree_kernel", "merkle_wg_kernel", "fri_fold", "compose"):
        assert any(want in r["demangled"] for r in rows), want
