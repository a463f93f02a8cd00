"""The tamper corpus of proofs over E (tests/verify_ext_corpus.py) on the CPU, no GPU needed: after the thinning every shape still has
every kind of field for both components, a "plus P" variant on a component-1 word, mostly rejections, and zk_verify_ext gives every item
the number of the plain-Python model ext_ref.verify.  tests/test_gpu_verify_ext.py holds the batched verifier to the same numbers."""
import pytest

import ext_ref
import verify_ext_corpus
from verify_ext_corpus import SHAPES, kind_of

IDS = ["-".join(str(int(v)) for v in s) for s in SHAPES]


def _c1_kinds(coset, D):
    return {"alpha#.c1", "beta#.c1", "coef#.c1" if D else "free_term.c1", "q#.g#.slot#.c1" if coset else "q#.g#.value#.c1"} | (set() if coset else {"q#.cp.c1"})


def _field_name(label):
    """p0.q1.g0.value2.c1.flip -> q1.g0.value2.c1"""
    parts = label.split(".")
    return ".".join(parts[1:-1])


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_kept_kind_and_a_plus_p_on_component_1(orc, shape, hash_kind):
    log_n, log_b, q, g, K, coset, D, c = shape
    ref = verify_ext_corpus.ref_objects(orc, *shape, hash_kind)[0]
    table = verify_ext_corpus.fields(ref, *shape)
    full = {kind_of(n) for n, _, _ in ext_ref.regions(*shape) if ".e" not in n and ".path" not in n}
    kinds = {kind_of(n) for n, _, _, _ in table}
    assert full <= kinds                                              # thinning drops no kind of value or count, so none for either component
    assert _c1_kinds(coset, D) <= kinds and all(k in verify_ext_corpus.KEPT_C1_KINDS for k in kinds if k.endswith(".c1"))
    assert {k[:-1] + "0" for k in kinds if k.endswith(".c1")} <= kinds
    assert any(k.endswith(".path#.node#") or k.endswith(".path.node#") for k in kinds) and "f_root.e#" in kinds and "root#.e#" in kinds
    caps = [n for n, _, _, _ in table if ".e" in n]
    assert c == 0 or any(not n.endswith(".e0") for n in caps), caps   # a cap is not always stood for by entry 0
    items = verify_ext_corpus.corpus(orc, *shape, hash_kind)
    assert len(items) <= 420, len(items)
    labels = [it.label for it in items]
    for k in _c1_kinds(coset, D):                                     # each kind reaches the corpus, flipped at least
        assert any(lb.endswith(".flip") and kind_of(_field_name(lb)) == k for lb in labels), k
    assert any(lb.endswith(".plusP") and _field_name(lb).endswith(".c1") for lb in labels), "no component-1 word w with w + P < 2^32: list other seeds in SHAPE_SEEDS"


@pytest.mark.parametrize("hash_kind", [0, 1], ids=["sha256", "field"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_zk_verify_ext_agrees_with_the_model_on_every_item(zk, orc, shape, hash_kind):
    log_n, log_b, q, g, K, coset, D, c = shape
    items = verify_ext_corpus.corpus(orc, *shape, hash_kind)
    for strict in (True, False):
        got = verify_ext_corpus.cpu_checks(zk.load(), items, *shape, hash_kind, strict)
        assert (got != 0).sum() > len(items) // 2                     # the corpus is mostly rejections
        assert got[[i for i, it in enumerate(items) if it.label.endswith(".valid")]].tolist() == [0, 0]
        for it, have in zip(items, got.tolist()):
            want = ext_ref.verify(orc, it.data, it.state if strict else None, log_n, log_b, it.public_last, hash_kind, q, g, K, coset, D, c)
            assert have == want, (it.label, strict, have, want)
        if not strict:                                                # without the replay, a changed component-1 word is still rejected
            for it, have in zip(items, got.tolist()):
                name = _field_name(it.label)
                if name.endswith(".c1") and it.label.endswith(".flip") and (name.startswith("q") or name.startswith("coef") or name.startswith("free_term")):
                    assert have != 0, it.label
