#!/usr/bin/env python3
"""Row leaves of the shared proof (zk_batch_set_shared_rows) against the shared proof without them: ms per statement at one
query and proof bytes at 1 and 32 queries, measured in ONE process and build.

Per size (8 x 2^24, 64 x 2^20, 256 x 2^13: statements x domain) and setting (K = 1 with one-value leaves; K = 3 with coset leaves) one
BatchContext with the seeds resident.  Before anything is timed both proofs are checked with the strict verifier; then a warm-up of both
settings, then blocks of calls INTERLEAVED over rows off and on, so that drift of the machine hits both alike.  A timed window is a run of
calls, each of which ends with its proof on the host.  ms per statement is the median over the blocks, the spread their minimum and
maximum.  The bytes are exact: zk_proof_data_len_shared and zk_proof_data_len_shared_rows (32 queries is more than the batched prover
takes, 16; the verifier and the format take 64).  The `counted` column is the SHA-256 compression count of DESIGN.md 7h for the trees of
one call, rows on over rows off -- a count, not a timing, printed beside the measured ratio; no ratio was fixed in advance.  One call in
flight at a time.

    python tools/batch_shared_rows_bench.py --out profiles/batch_shared_rows_bench.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((21, 3, 3), (17, 3, 6), (10, 3, 8))       # (log_n, log_blowup, log_batch)
SETTINGS = ((1, False), (3, True))                 # (fold_log, coset_leaves)
Q = 1


def fri_leaves(log_n, K, coset):
    """Leaves of the FRI trees of one proof (cp and every committed layer after it) in units of N."""
    total, r = 0.0, 0
    while r < log_n:
        steps = min(K, log_n - r)
        total += 2.0 ** -(r + (steps if coset else 0))
        r += steps
    return total + 2.0 ** -log_n                           # the last layer's tree


def compressions(log_n, lb, K, coset, rows):
    """SHA-256 compressions of the trees of ONE shared call in units of N: a tree of m leaves of <= 8 values is m leaf compressions and 2 m
    for its inner nodes; a row of M >= 16 values is M / 16 + 1."""
    M = 1 << lb
    fri = 3.0 * fri_leaves(log_n, K, coset)
    if not rows:
        return 3.0 * M + fri
    return (3.0 if M <= 8 else M / 16 + 3.0) + fri


def measure(zk, log_n, log_b, lb, K, coset, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    M = 1 << lb
    with zk.BatchContext(log_n, log_b, lb, queries=Q, fold_log=K, coset_leaves=coset) as bc:
        bc.gen_fibsq([1] * M, [3141592 + p for p in range(M)])
        lens = {rows: lib.zk_proof_data_len_shared_rows(log_n, log_b, Q, 0, K, int(coset), 0, 0, lb, int(rows)) for rows in (False, True)}
        data, state, got = np.zeros(max(lens.values()), dtype=np.uint8), np.zeros(32, dtype=np.uint8), C.c_size_t()

        def run(rows, count):
            bc.set_shared_rows(rows)
            t0 = time.perf_counter()
            for _ in range(count):
                rc = lib.zk_batch_prove_shared(bc._h, data.ctypes.data_as(C.c_void_p), lens[rows], C.byref(got), state.ctypes.data_as(C.c_void_p))
                if rc:
                    raise zk.ZkError(rc, lib.zk_last_error().decode())
            return time.perf_counter() - t0

        for rows in (False, True):
            bc.set_shared_rows(rows)
            assert bc.prove_shared().check(strict=True) == 0
        for rows in (False, True):
            run(rows, warmup)
        times = {False: [], True: []}
        for _ in range(blocks):
            for rows in (False, True):
                times[rows].append(run(rows, per_block) * 1e3 / (per_block * M))
    b32 = {rows: lib.zk_proof_data_len_shared_rows(log_n, log_b, 32, 0, K, int(coset), 0, 0, lb, int(rows)) for rows in (False, True)}
    return {"size": (log_n, log_b, lb), "K": K, "coset": coset, "off_ms": times[False], "on_ms": times[True], "b1": lens, "b32": b32,
            "counted": compressions(log_n, lb, K, coset, True) / compressions(log_n, lb, K, coset, False)}


def render(rows, build_hash, blocks, per_block, warmup):
    L = ["Shared proof with row leaves (zk_batch_set_shared_rows) beside the shared proof without, interleaved in one process and build (tools/batch_shared_rows_bench.py)",
         f"build {build_hash}, SHA-256, cap 0, no early stop; timed at {Q} query: blocks {blocks} x {per_block} calls per setting, warm-up {warmup} calls; one call in flight",
         "ms are PER STATEMENT; bytes are of the ONE proof of the batch, exact (the length formula); ratio: rows on over rows off;",
         "counted: SHA-256 compressions of the trees of a call, rows on over off (DESIGN.md 7h) -- a count, not a timing",
         "",
         "  statements x domain  K  leaves   rows off ms  [min .. max]           rows on ms  [min .. max]           ratio counted    off B q=1   on B q=1   off B q=32  on B q=32  ratio"]
    for r in rows:
        log_n, log_b, lb = r["size"]
        p, s = r["off_ms"], r["on_ms"]
        pm, sm = statistics.median(p), statistics.median(s)
        L.append(f"  {1 << lb:5d} x 2^{log_n + log_b:<2d}         {r['K']}  {'coset ' if r['coset'] else 'single'}  {pm:10.5f}  [{min(p):.5f} .. {max(p):.5f}]  "
                 f"{sm:10.5f}  [{min(s):.5f} .. {max(s):.5f}]  {sm / pm:5.3f}   {r['counted']:5.3f}   {r['b1'][False]:10d} {r['b1'][True]:10d}   "
                 f"{r['b32'][False]:10d} {r['b32'][True]:10d}  {r['b32'][True] / r['b32'][False]:5.3f}")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_shared_rows_bench.txt"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4, help="calls per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default=None, help="comma-separated indices into the three sizes (default: all)")
    ap.add_argument("--append", action="store_true", help="add to the file instead of replacing it")
    args = ap.parse_args()
    import zkstark_amd as zk
    from zkstark_amd import _lib
    sizes = SIZES if args.sizes is None else [SIZES[int(i)] for i in args.sizes.split(",")]
    rows = []
    for log_n, log_b, lb in sizes:
        for K, coset in SETTINGS:
            per = args.per_block if log_n > 12 else args.per_block * 16      # small domains: longer windows
            rows.append(measure(zk, log_n, log_b, lb, K, coset, args.blocks, per, args.warmup))
            print(f"{1 << lb} x 2^{log_n + log_b} K={K} done", flush=True)
    txt = render(rows, _lib.build_hash(), args.blocks, args.per_block, args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
