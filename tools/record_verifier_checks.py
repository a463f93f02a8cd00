"""Records the check numbers of the CPU verifier over the tamper corpora into tests/golden/verifier_checks.json, the file
tests/test_verifier_golden.py holds the verifier to.  It was written by the commit BEFORE the K = 1 and the folded verifier of
transcript.hpp were merged into one, so the numbers are those of the two separate verifiers.  Re-run it only when the wire
format or the corpus changes on purpose; two runs give the same bytes.

    python tools/record_verifier_checks.py [--check]      # --check: compare instead of write
"""
import ctypes as C
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden", "verifier_checks.json")

# (log_n, log_b, q): tests/verify_corpus.py, both hashes, K = 1 and no nonce
K1_SHAPES = [(4, 1, 1), (5, 2, 2)]
# (log_n, log_b, q, grind bits, K): tests/verify_fold_corpus.py, SHA-256
FOLD_SHAPES = [(5, 2, 2, 0, 2), (5, 2, 2, 8, 3), (7, 1, 1, 0, 3)]


def corpus_digest(items):
    """SHA-256 over every item's proof bytes, state and public_last: tells a drifting corpus from a drifting verifier."""
    h = hashlib.sha256()
    for it in items:
        h.update(it.data + it.state + struct.pack("<I", it.public_last))
    return h.hexdigest()


def shapes(orc):
    """(key dict, items) of every recorded shape, in file order."""
    import verify_corpus
    import verify_fold_corpus
    for log_n, log_b, q in K1_SHAPES:
        for hash_kind in (0, 1):
            yield (dict(log_n=log_n, log_b=log_b, q=q, g=0, K=1, hash=hash_kind), verify_corpus.corpus(orc, log_n, log_b, q, hash_kind))
    for log_n, log_b, q, g, K in FOLD_SHAPES:
        yield dict(log_n=log_n, log_b=log_b, q=q, g=g, K=K, hash=0), verify_fold_corpus.corpus(orc, log_n, log_b, q, g, K, 0)


def record(lib, orc):
    out = []
    for key, items in shapes(orc):
        rows = []
        for it in items:
            pair = []
            for state in (it.state, None):                               # strict, plain
                c = C.c_int32(12345)
                if key["K"] == 1:
                    lib.zk_verify_check(it.data, len(it.data), state, key["log_n"], key["log_b"], it.public_last, key["hash"], key["q"], C.byref(c))
                else:
                    lib.zk_verify_fold(it.data, len(it.data), state, key["log_n"], key["log_b"], it.public_last, key["hash"], key["q"], key["g"],
                                       key["K"], C.byref(c))
                pair.append(c.value)
            rows.append([it.label] + pair)
        out.append(dict(key, sha256=corpus_digest(items), rows=rows))
    return out


def dumps(shapes_out):
    lines = []
    for s in shapes_out:
        head = json.dumps({k: v for k, v in s.items() if k != "rows"})[:-1]
        lines.append(head + ', "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in s["rows"]) + "\n]}")
    return '{"shapes": [\n' + ",\n".join(lines) + "\n]}\n"


if __name__ == "__main__":
    import oracle
    import zkstark_amd
    text = dumps(record(zkstark_amd.load(), oracle))
    if "--check" in sys.argv:
        with open(OUT) as f:
            same = f.read() == text
        print("identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(OUT, len(text), "bytes,", sum(len(s["rows"]) for s in json.loads(text)["shapes"]), "rows")
