"""The Merkle planner mirror (tests/merkle_plans.py) and the grid of tests/test_gpu_merkle_plans.py, on the CPU: the grid must
reach every code path of the Merkle kernels that the planner can choose."""
import merkle_plans as mp
import pytest


@pytest.mark.parametrize("h", [mp.SHA, mp.FIELD])
def test_grid_reaches_every_form_the_planner_can_choose(h):
    reachable = mp.all_forms(h)
    missing = reachable - mp.grid_forms(h)
    assert not missing, f"the GPU grid misses {sorted(missing, key=str)}"
    # every form exists: the throughput launches of k = 1 .. 4 levels from the leaves and from inner nodes, and per phase of
    # merkle_wg_kernel every level form of the hash
    assert {("sub", kind, k) for kind in ("leaf", "inner") for k in range(1, mp.MAX_K + 1)} <= reachable
    level_forms = ("quad", "split", "lane") if h == mp.SHA else ("row", "quad", "lane")
    assert {(phase, f) for phase in (0, 1) for f in level_forms} <= reachable
    assert {("leaf", f) for f in (("lane",) if h == mp.SHA else ("row", "lane"))} == {f for f in reachable if f[0] == "leaf"}


def test_sha_one_lane_continuation_needs_a_raised_latency_log():
    """SHA-256's one-lane form in the continuation (more than 128 nodes per level left after phase 0) is never chosen with the
    latency log at 12 .. 17: there the cost model always ends phase 0 higher.  It is chosen for a 2^19-leaf tree at 19 and above
    (j = 10, j2 = 9), which the grid runs."""
    low = mp.all_forms(mp.SHA, lats=range(12, 18))
    assert (1, "lane") not in low and (1, "lane") in mp.all_forms(mp.SHA)
    assert mp.plan(19, mp.SHA, counter=True, lat=19) == [mp.Launch("wg", True, 19, 19, 10, 9)]


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
