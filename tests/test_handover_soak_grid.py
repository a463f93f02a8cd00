"""The grid of tests/test_gpu_handover_soak.py on the CPU: its rows reach the hand-overs they were chosen for (by the planner
mirror, tests/merkle_plans.py, which the GPU suite pins on the library's own profile), and the grinding lists meet the conditions
that make the batch grinder relaunch and compact its jobs."""
import handover_soak as hs
import merkle_plans as mp
import pytest

import grind_ref


def _union(h):
    out = []
    for r in hs.PROOF_ROWS:
        if r.h == h:
            out += [(r.id,) + la for la in hs.proof_launches(r)]
    return out


def _some(launches, pred):
    return [(rid, tree, la) for rid, tree, la, top, posts in launches if la.kind == "wg" and pred(la, top, posts)]


@pytest.mark.parametrize("h", [mp.SHA, mp.FIELD])
def test_proof_rows_reach_a_continuation_over_several_workgroups(h):
    """merkle_wg_kernel's phase 1: the last workgroup reads one node of every other workgroup (publish_node / load_digest_agent)."""
    assert _some(_union(h), lambda la, top, posts: la.j2 > 0 and hs.workgroups(la) > 1)


def test_proof_rows_reach_the_relaxed_mailbox_post():
    """j2 == 0, a hand-over depth and several workgroups: every workgroup publishes its node and the last one posts all 2^top to the
    host.  The launch that also posts the layer's values has the same shape but keeps the release / acquire form, so it is not
    counted here (it is the next test's)."""
    hits = _some(_union(mp.SHA), lambda la, top, posts: la.j2 == 0 and top > 0 and hs.workgroups(la) > 1 and la.depth - la.k == top and not posts)
    assert hits
    assert {rid for rid, _, _ in hits} >= {"sha256-13.3-default", "sha256-17.3-default", "sha256-13.3-default-fold3"}


def test_proof_rows_reach_the_launch_that_posts_layer_values():
    """The dump_src path.  The mirror has no such field; zkstark.hip's mail_of sets it for the tree (>= 1) over the layer of exactly
    2^(host_tail + 1) values, when the host finishes tree tops at all (host_top > 0), the hash is SHA-256 and the proof folds by 2:
    with the default host_levels (8, 9) that is the layer of 2^10 values, tree L - 9; with (5, 6) the layer of 2^7 values.  Every
    later round runs on the host thread, so the proof commits no smaller tree on the device."""
    for rid, tail, lg in (("sha256-13.3-default", 9, 10), ("sha256-13.3-host5.6", 6, 7), ("sha256-17.3-default", 9, 10)):
        row = next(r for r in hs.PROOF_ROWS if r.id == rid)
        assert row.effective_host_levels[1] == tail
        posting = [(tree, la, top) for tree, la, top, posts in hs.proof_launches(row) if posts]
        assert len(posting) == 1
        tree, la, top = posting[0]
        assert tree == row.log_n + row.log_b - lg + 1 and la.leaf and la.depth == lg and la.j2 == 0 and hs.workgroups(la) > 1
        assert max(t for t, _, _, _ in hs.proof_launches(row)) == tree        # the tail is the host's
    for r in hs.PROOF_ROWS:                                                     # and nowhere it should not be
        if r.h == mp.FIELD or r.fold_log != 1 or r.effective_host_levels == (0, 0):
            assert "posts values" not in hs.reach(hs.proof_launches(r)), r.id


def test_proof_rows_reach_a_launch_of_more_workgroups_than_cus():
    hits = _some(_union(mp.SHA), lambda la, top, posts: hs.workgroups(la) > hs.CUS)
    assert hits and all(la.j2 > 0 for _, _, la in hits)                        # ... whose last workgroup carries on
    # with the default latency log no merkle_wg_kernel launch of any proof is wider than the chip: hence the row that moves it
    assert all(hs.workgroups(la) <= hs.CUS for r in hs.PROOF_ROWS if r.lat == mp.LATENCY_LOG
               for _, la, _, _ in hs.proof_launches(r) if la.kind == "wg")


def test_proof_rows_are_the_issues_rows_with_their_floors():
    ids = [r.id for r in hs.PROOF_ROWS]
    assert len(set(ids)) == len(ids)
    for r in hs.PROOF_ROWS:
        assert r.pairs >= r.floor, r.id
    assert {"sha256-15.3-default", "field-15.3-default", "sha256-10.3-default-q7-grind14", "sha256-13.3-default-q2-early",
            "sha256-17.3-default-q2-early", "field-13.3-default-fold3", "sha256-17.3-default-fold3"} <= set(ids)
    # a throughput launch, then the latency phase
    row = next(r for r in hs.PROOF_ROWS if r.id == "sha256-15.3-default")
    assert [la.kind for _, la, _, _ in hs.proof_launches(row)][:2] == ["sub", "wg"]


def test_commit_cases_are_grid_cases_and_reach_both_hand_overs():
    seen = {}
    for h, log_m, lat, top, log_parts, pairs in hs.COMMIT_CASES:
        assert (log_m, lat, top, log_parts) in mp.commit_cases(h) and pairs >= hs.COMMIT_PAIRS_FLOOR
        assert log_m <= 16 or h == mp.SHA
        for what in hs.reach(hs.commit_launches(h, log_m, lat, top)):
            seen.setdefault(what, set()).add((h, top))
    assert {(mp.SHA, 3), (mp.SHA, 8)} <= seen["relaxed post"]
    assert {h for h, _ in seen["continuation"]} == {mp.SHA, mp.FIELD} and (mp.SHA, 3) in seen["continuation"]
    assert (mp.SHA, 13, 17, 3, 0) in [c[:5] for c in hs.COMMIT_CASES]
    assert mp.plan(19, mp.SHA, counter=True, lat=19) == [mp.Launch("wg", True, 19, 19, 10, 9)] and (mp.SHA, 19, 19, 0, 0) in [c[:5] for c in hs.COMMIT_CASES]
    assert any(c[4] > 0 for c in hs.COMMIT_CASES)


def test_proof_fields_cover_the_proof():
    import fold_ref
    for log_n, log_b, q, bits, K in ((10, 3, 1, 0, 1), (10, 3, 7, 14, 1), (13, 3, 2, 0, 3), (4, 1, 1, 12, 1), (6, 2, 1, 0, 3)):
        f = hs.proof_fields(log_n, log_b, q, bits, K)
        assert f[0][1] == 0 and all(a[2] == b[1] for a, b in zip(f, f[1:]))
        assert f[-1][2] == fold_ref.proof_len(log_n, log_b, q, bits, K)
    assert hs.proof_fields(10, 3)[-1][2] == __import__("verify_corpus").proof_len(10, 3, 1)
    assert hs.locate(0, 10, 3) == "root of tree 0 (f)" and hs.locate(80, 10, 3) == "root of tree 2"
    assert hs.first_difference(b"abcd" * 3000, b"abcd" * 3000) is None and hs.first_difference(b"a" * 5000 + b"b", b"a" * 5000 + b"c") == 5000


def test_grind_lists_make_the_batch_grinder_relaunch_and_compact(orc):
    """Re-derived with tests/grind_ref.py: at g = 12 the first launch covers the nonces below 2^14 (grind_chunk: the minimum chunk)."""
    log_n, log_b, log_batch, g = hs.GRIND_BATCH
    assert max(4 << g, 1 << 14) == hs.GRIND_FIRST_CHUNK
    assert hs.GRIND_LISTS[0] != hs.GRIND_LISTS[1]
    for a1s, slow_at in zip(hs.GRIND_LISTS, hs.GRIND_SLOW_AT):
        assert len(a1s) == 1 << log_batch == len(set(a1s))
        nonces = [grind_ref.grind_proof(orc, log_n, log_b, 1, 0, g, a1=a1)[3] for a1 in a1s]
        assert hs.grind_conditions(nonces) == (True, True, True), nonces
        assert tuple(p for p, w in enumerate(nonces) if w >= hs.GRIND_FIRST_CHUNK) == slow_at
