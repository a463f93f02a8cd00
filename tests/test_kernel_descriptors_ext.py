"""The kernels over E = F_P[u] / (u^2 - 5) (compose_ext_kernel / compose_ext_kernel4, fri_fold_multi_ext_kernel1 / fri_fold_multi_ext_kernel,
csrc/kernels.hip) as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): every instance exists once and keeps its loads and
its butterfly in registers -- no scratch, no LDS, no accumulation registers -- and the base-field kernels beside them are still found
under their names.  The register and instruction counts printed here are the ones DESIGN.md 7j records."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXT = (["compose_ext_kernel", "compose_ext_kernel4"]
       + [f"fri_fold_multi_ext_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_ext_kernel<{s}>" for s in (1, 2, 3)])
KEPT = (["compose_kernel", "compose_kernel4", "compose_batch_kernel", "compose_sum_batch_kernel", "fri_fold_kernel", "fri_fold_kernel4"]
        + [f"fri_fold_multi_kernel1<{s}>" for s in (1, 2, 3)] + [f"fri_fold_multi_kernel<{s}>" for s in (1, 2, 3)]
        + [f"fri_fold_multi_batch_kernel<{s}>" for s in (1, 2, 3)])


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


def test_every_ext_kernel_lives_in_registers(rows):
    for name in EXT:
        hit = _named(rows, name)
        assert len(hit) == 1, (name, [r["demangled"] for r in rows if "_ext_" in r["demangled"]])
        r = hit[0]
        print(f"{name}: vgpr {r['vgpr']} sgpr {r.get('sgpr')} valu {r.get('valu')} vmem {r.get('vmem')} total {r.get('total')}")
        assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0 and r["agpr"] == 0 and r.get("ds", 0) == 0, r
        assert 0 < r["vgpr"] <= 128 and r["valu"] > 0, r          # room for four waves per SIMD; the counts themselves are recorded, not pinned
    assert len([r for r in rows if "_ext_kernel" in r["demangled"]]) == len(EXT)


def test_a_value_of_compose_ext_costs_less_than_two_base_compositions(rows):
    """The operands and the three quotient terms are taken once: the static VALU count of each form stays well under twice its
    base-field namesake's (14 Montgomery multiplications against 2 x 11)."""
    for ext, base in (("compose_ext_kernel", "compose_kernel"), ("compose_ext_kernel4", "compose_kernel4")):
        e, b = _named(rows, ext)[0], _named(rows, base)[0]
        assert b["valu"] < e["valu"] <= 1.5 * b["valu"], (e["valu"], b["valu"])   # 14 / 11 = 1.27 by multiplications; 2.0 would be two passes
        assert e["vmem"] == b["vmem"] + 2, (e["vmem"], b["vmem"])      # the second plane's store and its zz look-up; no second read of f


def test_neighbouring_kernels_keep_their_names(rows):
    for name in KEPT:
        assert len(_named(rows, name)) == 1, (name, sorted(r["demangled"] for r in rows if name.split("<")[0] in r["demangled"]))
