"""The kernel that posts one heap level to the host (digest_level_post_kernel, csrc/kernels.hip: caps of a batch that the mailbox
cannot hold) as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): it exists, and it is the plain copy it promises to be --
no scratch, no LDS, no accumulation registers, a handful of vector registers.  The Merkle kernels the build launches in front of it
were not edited: they are still found under the names tests/test_kernel_descriptors.py looks for."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MERKLE_KERNELS = (["merkle_subtree_kernel<zk::PlainSrc, true, 0>", "merkle_subtree_kernel<zk::PlainSrc, false, 0>",
                   "merkle_subtree_kernel<zk::PlainSrc, true, 1>", "merkle_subtree_kernel<zk::PlainSrc, false, 1>"]
                  + [f"merkle_wg_kernel<zk::PlainSrc, {leaf}, {h}>" for leaf in ("true", "false") for h in (0, 1, 2)]
                  + [f"merkle_subtree_kernel<zk::{src}, true, {h}>" for src in ("ComposeBatchSrc", "FoldBatchSrc") for h in (0, 1)]
                  + [f"merkle_wg_kernel<zk::{src}, true, {h}>" for src in ("ComposeBatchSrc", "FoldBatchSrc") for h in (0, 1)]
                  + [f"coset_leaf_hash_batch_kernel<{h}, {s}>" for h in (0, 1) for s in (1, 2, 3)])


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


def test_post_kernel_is_a_plain_copy(rows):
    hit = _named(rows, "digest_level_post_kernel")
    assert len(hit) == 1, [r["demangled"] for r in rows if "post" in r["demangled"]]
    r = hit[0]
    assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0, r
    assert r["vgpr"] <= 32 and r.get("ds", 0) == 0, r          # a 16-byte load, a 16-byte store and their addresses


def test_merkle_kernels_keep_their_names(rows):
    for name in MERKLE_KERNELS:
        assert len(_named(rows, name)) == 1, (name, sorted(r["demangled"] for r in rows if name.split("<")[0] in r["demangled"]))
    for want in ("merkle_subtree_kernel", "merkle_wg_kernel"):   # the names tests/test_kernel_descriptors.py asks for
        assert any(want in r["demangled"] for r in rows), want
