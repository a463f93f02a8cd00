"""The kernels of the batch over E (compose_ext_batch_kernel / compose_ext_batch_kernel4, fri_fold_multi_ext_batch_prep_kernel /
_kernel1 / _kernel, coset_ext_leaf_hash_batch_kernel; csrc/kernels.hip) as built for gfx950 (no GPU needed; tools/kernel_descriptors.py):
every instance exists once, uses no scratch and no LDS and stays at or below 128 VGPRs, the count above which a SIMD holds fewer than four
waves; the base, batched and one-call ext kernels beside them are still found under their names.  The register and instruction counts
printed here are the ones DESIGN.md 7l records."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = (["compose_ext_batch_kernel", "compose_ext_batch_kernel4"]
       + [f"fri_fold_multi_ext_batch_prep_kernel<{s}>" for s in (1, 2, 3)]
       + [f"fri_fold_multi_ext_batch_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_ext_batch_kernel<{s}>" for s in (1, 2, 3)]
       + [f"coset_ext_leaf_hash_batch_kernel<{h}, {s}>" for h in (0, 1) for s in (1, 2, 3)])
KEPT = (["compose_kernel", "compose_kernel4", "compose_batch_kernel", "compose_sum_batch_kernel", "compose_ext_kernel", "compose_ext_kernel4"]
        + [f"fri_fold_multi_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_kernel<{s}>" for s in (1, 2, 3)]
        + [f"fri_fold_multi_batch_prep_kernel<{s}>" for s in (1, 2, 3)]
        + [f"fri_fold_multi_batch_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_batch_kernel<{s}>" for s in (1, 2, 3)]
        + [f"fri_fold_multi_ext_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_ext_kernel<{s}>" for s in (1, 2, 3)]
        + [f"coset_leaf_hash_batch_kernel<{h}, {s}>" for h in (0, 1) for s in (1, 2, 3)]
        + [f"row_leaf_hash_kernel<{h}, {lb}>" for h in (0, 1) for lb in range(1, 9)])


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


def test_every_new_kernel_lives_in_registers(rows):
    for name in NEW:
        hit = _named(rows, name)
        assert len(hit) == 1, (name, [r["demangled"] for r in rows if "ext_batch" in r["demangled"] or "coset_ext" in r["demangled"]])
        r = hit[0]
        print(f"{name}: vgpr {r['vgpr']} sgpr {r.get('sgpr')} valu {r.get('valu')} vmem {r.get('vmem')} total {r.get('total')}")
        assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0 and r.get("ds", 0) == 0, r
        assert 0 < r["vgpr"] <= 128 and r["valu"] > 0, r
    mine = [r for r in rows if "_ext_batch_" in r["demangled"].split("(")[0] or "coset_ext_leaf" in r["demangled"].split("(")[0]]
    assert len(mine) == len(NEW), sorted(r["demangled"] for r in mine)


def test_a_value_of_the_batched_composition_over_e_is_one_pass(rows):
    """Both planes from one read of f: the static VALU count stays well under twice the base batched kernel's (15 Montgomery
    multiplications against 2 x 12), and the wide form stores 16 bytes per plane as compose_ext_kernel4 does."""
    e, b = _named(rows, "compose_ext_batch_kernel")[0], _named(rows, "compose_batch_kernel")[0]
    assert b["valu"] < e["valu"] <= 1.5 * b["valu"], (e["valu"], b["valu"])
    w, o = _named(rows, "compose_ext_batch_kernel4")[0], _named(rows, "compose_ext_kernel4")[0]
    assert w["valu"] <= 1.25 * o["valu"], (w["valu"], o["valu"])      # the one-call form plus four products by alpha2 and the proof index


def test_neighbouring_kernels_keep_their_names(rows):
    for name in KEPT:
        assert len(_named(rows, name)) == 1, (name, sorted(r["demangled"] for r in rows if name.split("<")[0] in r["demangled"]))
