"""Batches and tamper corpora of shared proofs for the batched GPU verifier (tests/test_gpu_verify_shared.py).

The proofs are built without the library (tests/shared_ref.py, with row leaves tests/rows_ref.py), two per shape: first=SEED and another
seed.  What a batch or a variant is expected to give is always the library's CPU verifier, zk_verify_shared_rows (cpu_checks), which
tests/test_shared_fri.py and tests/test_shared_rows.py tie to the Python models.

A corpus is one flipped bit per region of regions(); where a shape has more than ~300 regions every n-th one is kept, together with the
first region of every kind in required_kinds(), so that a thinned corpus still touches every piece of the format."""
import ctypes as C
import functools
import re

import numpy as np

import rows_ref
import shared_ref

SEED = shared_ref.SEED
OTHER_SEED = SEED + 4099
MAX_REGIONS = 300

# (log_n, log_b, lb, K, coset, D, c, q, hash, grind bits, the row-leaf settings the shape runs with)
SHAPES = [
    (2, 1, 1, 1, False, 0, 8, 1, 0, 0, (False, True)),   # L = 3, ce_f = 2: paths of one digest, an f commitment of 2^(lb + ce_f) digests
    (4, 1, 3, 2, True, 1, 0, 2, 0, 0, (False, True)),    # lb 3: a row is one compression; K > 1, coset, D > 0, cap 0
    (5, 2, 4, 3, True, 2, 2, 2, 0, 0, (False, True)),    # lb 4: a row is streamed blocks; cap > 0
    (4, 2, 4, 1, False, 0, 2, 2, 1, 0, (False, True)),   # the field hash's chain of two
    (4, 1, 8, 2, False, 0, 1, 1, 0, 0, (False, True)),   # 256 statements: 16 + 1 SHA-256 blocks; (proof, statement) lanes span many waves
    (4, 1, 8, 1, True, 0, 0, 1, 1, 0, (False, True)),    # 256 statements: a field chain of 32
    (6, 3, 6, 2, False, 0, 2, 2, 0, 0, (False,)),        # 64 statements: one wave per proof
    (4, 1, 2, 1, False, 0, 1, 2, 0, 6, (False, True)),   # grinding: the nonce replay
]


def shape_id(s):
    return "-".join(str(int(v)) for v in s[:10])


class Item:
    """One shared proof to check: its bytes, the channel state, the public values of its statements, and what was done to it."""

    def __init__(self, label, data, state, public_last):
        self.label, self.data, self.state = label, bytes(data), bytes(state)
        self.public_last = [int(v) & 0xFFFFFFFF for v in public_last]


def _ref(rows):
    return rows_ref if rows else shared_ref


@functools.lru_cache(maxsize=64)
def ref_proofs(orc, shape, rows):
    """The two valid proofs of a shape, [(data, state, public_last list)]."""
    log_n, log_b, lb, K, coset, D, c, q, h, g = shape[:10]
    out = []
    for first in (SEED, OTHER_SEED):
        r = _ref(rows).proof(orc, log_n, log_b, lb, q, h, K, coset, D, c, bits=g, first=first)
        out.append((r.data, r.state, list(r.public_last)))
    return out


def regions(shape, rows):
    log_n, log_b, lb, K, coset, D, c, q, h, g = shape[:10]
    return _ref(rows).regions(log_n, log_b, q, g, K, coset, D, c, lb)


def cpu_check(lib, data, state, public_last, log_n, log_b, lb, K, coset, D, c, q, h, g, rows):
    """The check number of the CPU verifier for one proof: zk_verify_shared_rows, or zk_verify_cap's for lb = 0 (one public value)."""
    n = C.c_int32(12345)
    if lb == 0:
        rc = lib.zk_verify_cap(data, len(data), state, log_n, log_b, int(public_last[0]) & 0xFFFFFFFF, h, q, g, K, int(bool(coset)), D, c, C.byref(n))
    else:
        arr = np.ascontiguousarray(public_last, dtype=np.uint32)
        rc = lib.zk_verify_shared_rows(data, len(data), state, log_n, log_b, arr.ctypes.data_as(C.c_void_p), lb, h, q, g, K, int(bool(coset)), D, c,
                                       int(bool(rows)), C.byref(n))
    assert rc == (0 if n.value == 0 else -6), (rc, n.value)
    return n.value


def cpu_checks(lib, items, shape, rows, strict):
    """The CPU verifier's number for every item, as an int32 array."""
    return np.array([cpu_check(lib, it.data, it.state if strict else None, it.public_last, *shape[:10], rows) for it in items], dtype=np.int32)


def valid_batch(orc, shape, rows, count):
    """count items, the two valid proofs in turn; the last one has one byte of its last path flipped."""
    proofs = ref_proofs(orc, shape, rows)
    items = [Item(f"p{i}", *proofs[i & 1]) for i in range(count)]
    d = bytearray(items[-1].data)
    d[-5] ^= 4
    items[-1] = Item(f"p{count - 1}.bad", bytes(d), items[-1].state, items[-1].public_last)
    return items


# ---- the tamper corpus -----------------------------------------------------------------------------------------------------------
_KIND = [
    (re.compile(r"^(s\d+\.)?f_root\.e\d+$"), "f_commitment"),
    (re.compile(r"^s\d+\.alpha\d$"), "alpha"),
    (re.compile(r"^root\d+\.e\d+$"), "root"),
    (re.compile(r"^beta\d+$"), "beta"),
    (re.compile(r"^(free_term|coef\d+)$"), "final"),
    (re.compile(r"^nonce$"), "nonce"),
    (re.compile(r"^raw\d+$"), "raw"),
]


def _where(M):
    """statement -> "first" / "middle" / "last" (two statements have no middle one)."""
    return {0: "first", M // 2: "middle", M - 1: "last"}


def kind_of(name, M):
    """The kind of a region: what required_kinds() asks for, or a kind nothing asks for."""
    for rx, kind in _KIND:
        if rx.match(name):
            return kind
    where = _where(M)
    m = re.match(r"^q\d+\.s(\d+)\.f(\d)\.(value|count|path)$", name)
    if m:                                                 # plain shared: the tuple of statement p's f(g^i x)
        p = int(m.group(1))
        return f"f{m.group(2)}.{m.group(3)}.{where[p]}" if p in where else "f.other"
    m = re.match(r"^q\d+\.row(\d)\.value(\d+)$", name)
    if m:                                                 # rows: value p of row i
        p = int(m.group(2))
        return f"row{m.group(1)}.value.{where[p]}" if p in where else "row.other"
    m = re.match(r"^q\d+\.row(\d)\.(count|path)$", name)
    if m:
        return f"row{m.group(1)}.{m.group(2)}"
    m = re.match(r"^q\d+\.f3\.(value|count|path)$", name)
    if m:
        return f"cp.{m.group(1)}"
    m = re.match(r"^q\d+\.g(\d+)\.(slot|value|count|path)\d*$", name)
    if m:
        return f"g{m.group(1)}.{'value' if m.group(2) == 'slot' else m.group(2)}"
    raise AssertionError(f"a region of no known kind: {name}")


def required_kinds(shape, rows):
    """What a corpus must touch: an f-commitment entry, an alpha, the value, count and path of an f / row tuple of the first, a middle and
    the last statement (a row has one count and one path for all), the cp tuple, a value and a path of every group, the final term or the
    coefficients, the nonce, a raw."""
    log_n, log_b, lb, K, coset, D, c, q, h, g = shape[:10]
    G = (log_n - D + K - 1) // K
    need = {"f_commitment", "alpha", "final", "raw"} | ({"nonce"} if g else set())
    for i in range(3):
        for w in set(_where(1 << lb).values()):
            need |= {f"row{i}.value.{w}"} if rows else {f"f{i}.value.{w}", f"f{i}.count.{w}", f"f{i}.path.{w}"}
        if rows:
            need |= {f"row{i}.count", f"row{i}.path"}
    if not coset:
        need |= {"cp.value", "cp.count", "cp.path"}
    for j in range(G):
        need |= {f"g{j}.value", f"g{j}.path"}
    return need


def kept_regions(shape, rows):
    """Every region, or every n-th one and the first of each required kind where there are more than MAX_REGIONS."""
    regs, M = regions(shape, rows), 1 << shape[2]
    need = required_kinds(shape, rows)
    n = (len(regs) + MAX_REGIONS - 1) // MAX_REGIONS
    keep, seen = [], set()
    for i, r in enumerate(regs):
        kind = kind_of(r[0], M)
        if i % n == 0 or (kind in need and kind not in seen):
            keep.append(r)
        seen.add(kind)
    have = {kind_of(r[0], M) for r in keep}
    assert need <= have, sorted(need - have)
    return keep


def corpus(orc, shape, rows):
    """The two valid proofs; one bit flipped in each kept region of the first; the first proof cut at the front and at the back (padded with
    zeros to its length) and padded at the front; public_last swapped between two statements; a wrong state; zeros."""
    proofs = ref_proofs(orc, shape, rows)
    data, state, last = proofs[0]
    out = [Item(f"p{i}.valid", *p) for i, p in enumerate(proofs)]
    for name, off, size in kept_regions(shape, rows):
        bit = (off * 7 + 3) % (8 * size)
        d = bytearray(data)
        d[off + bit // 8] ^= 1 << (bit % 8)
        out.append(Item(f"p0.{name}.flip", bytes(d), state, last))
    n = len(data)
    out.append(Item("p0.cut_front", data[4:] + bytes(4), state, last))
    out.append(Item("p0.cut_back", data[:n - 40] + bytes(40), state, last))
    out.append(Item("p0.padded_front", (bytes(4) + data)[:n], state, last))
    swapped = list(last)
    swapped[0], swapped[-1] = swapped[-1], swapped[0]
    out.append(Item("p0.public_last.swap", data, state, swapped))
    bad_state = bytearray(state)
    bad_state[5] ^= 0x10
    out.append(Item("p0.state", data, bytes(bad_state), last))
    out.append(Item("zeros", bytes(n), bytes(32), [0] * len(last)))
    return out


def expected_numbers(want, coset):
    """The issue's list: the distinct check numbers a corpus must produce (strict and not together)."""
    have = set(int(v) for v in want)
    missing = [n for n in (-2, -4, -5, -6) + (() if coset else (-7,)) if n not in have]
    if not any(-200 < v <= -100 for v in have):
        missing.append("-(100+j)")
    if not any(-400 < v <= -300 for v in have):
        missing.append("-(300+j)")
    if not coset and not any(-500 < v <= -400 for v in have):
        missing.append("-(400+j)")
    if not any(v <= -1000 for v in have):
        missing.append("<= -1000")
    return missing
