"""The Merkle planner mirror (tests/merkle_plans.py) and the grid of tests/test_gpu_merkle_plans.py, on the CPU: the grid must
reach every code path of the Merkle kernels that the planner can choose."""
import os
import re

import merkle_plans as mp
import pytest

LEVEL_FORMS = {mp.SHA: ("quad", "split", "lane"), mp.FIELD: ("row", "quad", "lane"), mp.B2S: ("lane", "lane2")}
LEAF_FORMS = {mp.SHA: ("lane",), mp.FIELD: ("row", "lane"), mp.B2S: ("lane", "lane4")}


@pytest.mark.parametrize("h", [mp.SHA, mp.FIELD, mp.B2S])
def test_grid_reaches_every_form_the_planner_can_choose(h):
    reachable = mp.all_forms(h)
    missing = reachable - mp.grid_forms(h)
    assert not missing, f"the GPU grid misses {sorted(missing, key=str)}"
    # every form exists: the throughput launches of k = 1 .. 4 levels from the leaves and from inner nodes, and per phase of
    # merkle_wg_kernel every level form of the hash
    assert {("sub", kind, k) for kind in ("leaf", "inner") for k in range(1, mp.MAX_K + 1)} <= reachable
    assert {(phase, f) for phase in (0, 1) for f in LEVEL_FORMS[h]} <= reachable
    assert {("leaf", f) for f in LEAF_FORMS[h]} == {f for f in reachable if f[0] == "leaf"}
    # BLAKE2s names the first loads too: of an inner-mode launch and of the continuation, within and beyond one input per thread
    loads = {("load", phase, n) for phase in (0, 1) for n in ("one", "many")} if h == mp.B2S else set()
    assert loads == {f for f in reachable if f[0] == "load"}


def test_sha_one_lane_continuation_needs_a_raised_latency_log():
    """SHA-256's one-lane form in the continuation (more than 128 nodes per level left after phase 0) is never chosen with the
    latency log at 12 .. 17: there the cost model always ends phase 0 higher.  It is chosen for a 2^19-leaf tree at 19 and above
    (j = 10, j2 = 9), which the grid runs."""
    low = mp.all_forms(mp.SHA, lats=range(12, 18))
    assert (1, "lane") not in low and (1, "lane") in mp.all_forms(mp.SHA)
    assert mp.plan(19, mp.SHA, counter=True, lat=19) == [mp.Launch("wg", True, 19, 19, 10, 9)]


def test_blake2s_wide_continuation_needs_a_raised_latency_log():
    """BLAKE2s: a continuation over more than 256 nodes -- its first load with several digests per thread, and with 2^10 nodes a
    level of 512 where a thread hashes two -- is never chosen with the latency log at 12 .. 17: phase 0 then leaves at most 2^8
    nodes.  The load is reached by a 2^19-leaf tree at 19 (j = 10, j2 = 9), the two-node level by a 2^20-leaf tree at 20 (j = 10,
    j2 = 10), the smallest trees that do; the grid runs both on a context."""
    low, every = mp.all_forms(mp.B2S, lats=range(12, 18)), mp.all_forms(mp.B2S)
    assert every - low == {("load", 1, "many"), (1, "lane2")}
    assert mp.plan(19, mp.B2S, counter=True, lat=19) == [mp.Launch("wg", True, 19, 19, 10, 9)]
    assert mp.plan(20, mp.B2S, counter=True, lat=20) == [mp.Launch("wg", True, 20, 20, 10, 10)]
    assert mp.B2S_RAISED_CASES == [(19, 19), (20, 20)]
    for form, first in ((("load", 1, "many"), 19), ((1, "lane2"), 20)):
        hits = [log_m for log_m in range(21) if any(form in mp.forms(mp.plan(log_m, mp.B2S, True, 0, lat, leaf_mode=lm), mp.B2S)
                                                    for lat in range(12, 25) for lm in (True, False))]
        assert hits[0] == first, (form, hits)


def test_blake2s_cost_entries_are_the_header_constants():
    """kB2sLevelUs / kB2sLeafUs (kernels.hip) are built from four instruction counts of csrc/kernels.hpp; the mirror's copies are
    those numbers, combined in the same order (the planner compares costs with a strict <)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "zkstark_amd", "csrc", "kernels.hpp")) as f:
        text = f.read()
    got = {name: float(v) for name, v in re.findall(r"constexpr double (k\w+Ops) = ([0-9.]+);", text)}
    assert (got["kB2sInnerOps"], got["kShaInnerOps"], got["kB2sLeafOps"], got["kShaLeafOps"]) == \
        (mp.B2S_INNER_OPS, mp.SHA_INNER_OPS, mp.B2S_LEAF_OPS, mp.SHA_LEAF_OPS)
    assert mp.B2S_LEVEL_US == got["kB2sInnerOps"] * 4.6 / got["kShaInnerOps"]
    assert mp.B2S_LEAF_US == got["kB2sLeafOps"] * 2.6 / got["kShaLeafOps"]
    with open(os.path.join(root, "zkstark_amd", "csrc", "kernels.hip")) as f:
        hip = f.read()
    assert "kB2sLevelUs = kB2sInnerOps * 4.6 / kShaInnerOps, kB2sLeafUs = kB2sLeafOps * 2.6 / kShaLeafOps;" in hip


def test_mirror_reproduces_the_documented_plans():
    """Plans the kernels.hip comments and the round notes describe: Merkle.new (no counter) at 2^12 leaves runs two plain
    launches of six levels, a proof's tree (a counter) one launch with a continuation.  (Whether the library really runs what
    the mirror says is checked on the GPU, from its profile: tests/test_gpu_merkle_plans.py.)"""
    assert [(la.k, la.j2) for la in mp.plan(12, mp.SHA)] == [(6, 0), (6, 0)]
    assert [(la.k, la.j2) for la in mp.plan(12, mp.SHA, counter=True)] == [(5, 7)]
    # throughput launches down to 2^lat nodes, then the latency phase
    p = mp.plan(22, mp.SHA, counter=True, top=8)
    assert [(la.kind, la.leaf, la.k) for la in p[:2]] == [("sub", True, 4), ("sub", False, 1)]
    assert p[2].kind == "wg" and p[2].span == 17 and p[2].k + p[2].j2 == 17 - 8
    # a chunk build of a large tree is one throughput launch of <= 3 levels; the finish starts where it stopped
    chunks, fin = mp.chunk_plans(18, 4, mp.SHA, lat=13)
    assert all(c == [mp.Launch("sub", True, 18, 14, 3)] for c in chunks) and fin[0].depth == 15 and not fin[0].leaf
    # BLAKE2s has cost entries of its own, so splits of its own: whole trees with a counter at the default switch ...
    splits = {10: (3, 7), 11: (6, 5), 12: (6, 6), 13: (5, 8), 14: (6, 8), 15: (7, 8), 16: (8, 8), 17: (9, 8)}
    for log_m, split in splits.items():
        assert mp.plan(log_m, mp.B2S, counter=True) == [mp.Launch("wg", True, log_m, log_m, *split)]
    # ... and in inner mode below one throughput launch (the switch at the inner tree's size)
    inner = {12: (4, 8), 13: (5, 8), 14: (9, 5), 15: (9, 6), 16: (8, 8), 17: (9, 8)}
    for lat, split in inner.items():
        assert mp.plan(lat + 1, mp.B2S, counter=True, lat=lat) == [mp.Launch("sub", True, lat + 1, lat + 1, 1), mp.Launch("wg", False, lat, lat, *split)]
        assert mp.plan(lat, mp.B2S, counter=True, leaf_mode=False) == [mp.Launch("wg", False, lat, lat, *split)]
    # no counter (Merkle.new): plain launches of <= 10 levels, whatever the hash
    assert [(la.k, la.j2) for la in mp.plan(12, mp.B2S)] == [(6, 0), (6, 0)]
    # a proof's 2^18-leaf tree: one throughput level, then the largest tree the latency kernel takes alone
    assert mp.plan(18, mp.B2S, counter=True) == [mp.Launch("sub", True, 18, 18, 1), mp.Launch("wg", False, 17, 17, 9, 8)]
