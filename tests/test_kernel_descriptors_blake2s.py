"""The BLAKE2s kernels as built for gfx950 (no GPU needed; tools/kernel_descriptors.py): which instances exist, their registers, and
the instruction counts kernels.hpp quotes (kB2sLeafOps, kB2sInnerOps).  The derived bounds say how the hash must have
compiled: the rounds unrolled with the message words in registers, every rotation one v_alignbit_b32."""
import importlib.util
import os
import re
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def kd():
    mod = _load("kernel_descriptors", os.path.join(ROOT, "tools", "kernel_descriptors.py"))
    if not os.path.exists(os.path.join(mod.LLVM, "llvm-readelf")):
        pytest.skip("llvm tools not present")
    from zkstark_amd import _lib
    _lib.load()                                   # builds the library if needed
    return mod


@pytest.fixture(scope="module")
def rows(kd):
    return kd.collect(want_isa=True)


def _hpp(name):
    hpp = open(os.path.join(ROOT, "zkstark_amd", "csrc", "kernels.hpp")).read()
    return float(re.search(name + r"\s*=\s*([0-9.]+)", hpp).group(1))


def test_the_four_throughput_instances(rows):
    """Plain / Compose / Fold leaves and the inner mode: what the one-call prover reaches.  No scratch, no AGPRs, and at most 128
    VGPRs: the four waves per SIMD that 40 KiB of LDS per workgroup allow (the reasoning of the field-hash bound)."""
    sub = [r for r in rows if "b2s_subtree_kernel<" in r["demangled"]]
    got = sorted(re.search(r"b2s_subtree_kernel<(.*?)>\(", r["demangled"] + "(").group(1) for r in sub)
    assert got == ["zk::ComposeSrc, true", "zk::FoldSrc, true", "zk::PlainSrc, false", "zk::PlainSrc, true"], got
    for r in sub:
        assert r.get("scratch", 0) == 0 and r["agpr"] == 0 and r["vgpr"] <= 128, (r["demangled"], r.get("scratch"), r["agpr"], r["vgpr"])


def test_the_other_instances_exist_and_do_not_spill(rows):
    names = [r["demangled"] for r in rows]
    for want in ("merkle_wg_kernel<zk::PlainSrc, true, 2>", "merkle_wg_kernel<zk::PlainSrc, false, 2>", "merkle_wg_kernel<zk::ComposeSrc, true, 2>",
                 "merkle_wg_kernel<zk::FoldSrc, true, 2>", "hash_chain_probe_kernel<2>", "coset_leaf_hash_kernel<2, 1>",
                 "coset_leaf_hash_kernel<2, 2>", "coset_leaf_hash_kernel<2, 3>"):
        hit = [r for r in rows if want in r["demangled"]]
        assert len(hit) == 1, (want, [n for n in names if "2>" in n])
        assert hit[0].get("scratch", 0) == 0 and hit[0]["vgpr"] <= 256, hit[0]


def _kernel(kd, substring):
    """(loops, disassembly) of the one kernel whose demangled name contains `substring`."""
    with tempfile.TemporaryDirectory() as td:
        for i, elf in enumerate(kd.code_objects(kd.fatbin_bytes())):
            path = os.path.join(td, f"co{i}.elf")
            with open(path, "wb") as f:
                f.write(elf)
            for k in kd.notes(path):
                if substring in kd.demangle([k["name"]])[k["name"]]:
                    dis = kd._disasm(path)
                    m = re.search(r"^([0-9a-f]+) <" + re.escape(k["name"]) + r">:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.S | re.M)
                    return kd.loops(path, k["name"]), int(m.group(1), 16), m.group(2)
    raise AssertionError(substring + " not found")


def _ops_between(base, text, lo, hi):
    """Mnemonics of the instructions at kernel-relative offsets lo .. hi."""
    ops = []
    for line in text.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)\b.*//\s*([0-9A-Fa-f]+):", line)
        if m and lo <= int(m.group(2), 16) - base <= hi:
            ops.append(m.group(1))
    return ops


def test_instruction_counts_quoted_by_kernels_hpp(kd):
    """The chain probe's loop body is one inner hash; the loops of b2s_subtree_kernel<PlainSrc, true> are one leaf hash and one inner
    hash with their addressing: within 25 instructions of kB2sLeafOps / kB2sInnerOps, the allowance of the SHA-256 test."""
    leaf_ops, inner_ops = _hpp("kB2sLeafOps"), _hpp("kB2sInnerOps")
    probe, _, _ = _kernel(kd, "hash_chain_probe_kernel<2>")
    assert len(probe) == 1 and abs(probe[0][2] - inner_ops) <= 25, (probe, inner_ops)
    loops, _, _ = _kernel(kd, "b2s_subtree_kernel<zk::PlainSrc, true>")
    counts = sorted(l[2] for l in loops)
    assert [c for c in counts if abs(c - leaf_ops) <= 25] and [c for c in counts if abs(c - inner_ops) <= 25], (counts, leaf_ops, inner_ops)
    assert leaf_ops < inner_ops                  # a leaf's zero message words fold away


def test_inner_loop_is_eighty_g_functions_and_nothing_else(kd):
    """Derived, not measured: a G is 14 two-operand operations before any fusing (4 additions with a message word in two of them = 6
    adds, 4 xors, 4 rotations), a compression has 80 of them, and setup, finalisation, the byte swaps of blake2s.hpp's boundary and
    the addressing fit in 64 more.  More means the rotations or the message indexing compiled badly.  The 320 rotations are one
    instruction each; byte permutes appear only as the 24 byte swaps (16 message words in, 8 digest words out)."""
    loops, base, text = _kernel(kd, "b2s_subtree_kernel<zk::PlainSrc, true>")
    inner_ops = _hpp("kB2sInnerOps")
    cand = [l for l in loops if abs(l[2] - inner_ops) <= 25]
    assert cand, loops
    lo, hi, n = min(cand, key=lambda l: l[1] - l[0])
    assert n <= 80 * 14 + 64, n
    ops = _ops_between(base, text, lo, hi)
    rot, perm = ops.count("v_alignbit_b32"), ops.count("v_perm_b32")
    assert rot + perm == 320 + 24 and rot <= 320, (rot, perm)   # a permute may stand in for a rotation by 16 or 8, never the reverse
    assert not [o for o in ops if o.startswith(("scratch_", "buffer_"))], "the message words must stay in registers"
    # the probe: the same hash without memory traffic
    ploops, pbase, ptext = _kernel(kd, "hash_chain_probe_kernel<2>")
    pops = _ops_between(pbase, ptext, ploops[0][0], ploops[0][1])
    assert pops.count("v_alignbit_b32") == 320 and len([o for o in pops if o.startswith("v_")]) <= 80 * 14 + 64
