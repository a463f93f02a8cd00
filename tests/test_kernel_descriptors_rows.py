"""The leaf kernel of the shared proof's row leaves (row_leaf_hash_kernel, csrc/kernels.hip) as built for gfx950 (no GPU needed;
tools/kernel_descriptors.py): every instance -- SHA-256 and the field hash, 2 .. 256 values per row -- exists once, keeps the two message
blocks, the chaining state and the schedule in registers (no scratch, no LDS, no accumulation registers), and its vector register count
and instruction count are the ones DESIGN.md 7h records.  The Merkle kernels around it were not edited: they are still found under the
names the other descriptor tests look for."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# VGPRs as built.  SHA-256 streams 16 + 16 message words, 8 state words and the round variables; the field hash holds its
# 16-element state in double precision (32 registers) beside 8 + 8 message words, as coset_leaf_hash_kernel<1, *> does.
VGPR_RECORDED = {(0, 1): 51, (0, 2): 53, (0, 3): 57, (0, 4): 52, (0, 5): 60, (0, 6): 60, (0, 7): 60, (0, 8): 60,
                 (1, 1): 122, (1, 2): 100, (1, 3): 112, (1, 4): 118, (1, 5): 118, (1, 6): 118, (1, 7): 118, (1, 8): 118}
# Static VALU instructions: a streamed SHA-256 leaf kernel is ONE data compression and the folded padding compression whatever M -- the
# block loop is not unrolled -- so the count must not grow with the row from LB = 5 on (LB = 4 has a single data block and no block loop)
VALU_LIMIT = {0: 2600, 1: 1600}

KEPT = ([f"coset_leaf_hash_kernel<{h}, {s}>" for h in (0, 1, 2) for s in (1, 2, 3)]
        + [f"coset_leaf_hash_batch_kernel<{h}, {s}>" for h in (0, 1) for s in (1, 2, 3)]
        + ["merkle_subtree_kernel<zk::PlainSrc, true, 0>", "merkle_subtree_kernel<zk::PlainSrc, false, 0>",
           "merkle_subtree_kernel<zk::PlainSrc, false, 1>", "compose_sum_batch_kernel", "digest_level_post_kernel"])


@pytest.fixture(scope="module")
def rows():
    spec = importlib.util.spec_from_file_location("kernel_descriptors", os.path.join(ROOT, "tools", "kernel_descriptors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(os.path.join(mod.LLVM, "llvm-readelf")):
        pytest.skip("llvm tools not present")
    from zkstark_amd import _lib
    _lib.load()                                   # builds the library if needed
    return mod.collect(want_isa=True)


def _named(rows, want):
    return [r for r in rows if r["demangled"].endswith("::" + want) or ("::" + want + "(") in r["demangled"]]


def test_every_row_leaf_kernel_lives_in_registers(rows):
    for h in (0, 1):
        for lb in range(1, 9):
            hit = _named(rows, f"row_leaf_hash_kernel<{h}, {lb}>")
            assert len(hit) == 1, (h, lb, [r["demangled"] for r in rows if "row_leaf" in r["demangled"]])
            r = hit[0]
            print(f"row_leaf_hash_kernel<{h}, {lb}>: vgpr {r['vgpr']} sgpr {r.get('sgpr')} valu {r.get('valu')} vmem {r.get('vmem')} total {r.get('total')}")
            assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0 and r.get("ds", 0) == 0, r
            assert r["vgpr"] <= VGPR_RECORDED[(h, lb)], r
            assert 0 < r["valu"] <= VALU_LIMIT[h], r
    assert len([r for r in rows if "row_leaf_hash_kernel" in r["demangled"]]) == 16   # no BLAKE2s instance


def test_a_streamed_leaf_is_one_compression_whatever_the_row(rows):
    for h in (0, 1):
        valu = [_named(rows, f"row_leaf_hash_kernel<{h}, {lb}>")[0]["valu"] for lb in range(5, 9)]
        assert max(valu) - min(valu) <= 16, (h, valu)


def test_neighbouring_kernels_keep_their_names(rows):
    for name in KEPT:
        assert len(_named(rows, name)) == 1, (name, sorted(r["demangled"] for r in rows if name.split("<")[0] in r["demangled"]))
