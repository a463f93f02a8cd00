#!/usr/bin/env python3
"""The shared proof of the batched prover against zk_batch_prove: ms per statement and proof bytes per statement, measured in ONE process
and build.

Per size (8 x 2^24, 64 x 2^20, 256 x 2^13: statements x domain) and setting (K = 1 with one-value leaves; K = 3 with coset leaves) one
BatchContext with the seeds resident.  Before anything is timed the shared proof is checked with the strict verifier (zk_verify_shared)
and one proof of the batch with its own; then a warm-up of both entry points, then blocks of calls INTERLEAVED over the two, so that drift
of the machine hits both alike.  A timed window is a run of calls, each of which ends with its proofs on the host.  ms per statement is
the median over the blocks, the spread their minimum and maximum.  Bytes are zk_proof_data_len_cap's and zk_proof_data_len_shared's / M.
The hash-count column is the model of DESIGN.md 7g: leaf hashes of the committed trees per statement, shared over separate -- a count,
not a timing.  One call in flight at a time.

    python tools/batch_shared_bench.py --out profiles/batch_shared_bench.txt
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


def leaf_hashes(log_n, log_b, K, coset):
    """Leaf hashes of one statement's FRI trees (cp and every committed layer after it) in units of N: the f tree is 1."""
    total, r = 0.0, 0
    while r < log_n:
        steps = min(K, log_n - r)
        total += 2.0 ** -(r + (steps if coset else 0))
        r += steps
    return total + 2.0 ** -log_n                           # the last layer's tree


def measure(zk, log_n, log_b, lb, K, coset, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    M = 1 << lb
    with zk.BatchContext(log_n, log_b, lb, queries=Q, fold_log=K, coset_leaves=coset) as bc:
        bc.gen_fibsq([1] * M, [3141592 + p for p in range(M)])
        plen = lib.zk_proof_data_len_cap(log_n, log_b, Q, 0, K, int(coset), 0, 0)
        slen = lib.zk_proof_data_len_shared(log_n, log_b, Q, 0, K, int(coset), 0, 0, lb)
        data, states = np.zeros((M, plen), dtype=np.uint8), np.zeros((M, 32), dtype=np.uint8)
        sdata, sstate, got = np.zeros(slen, dtype=np.uint8), np.zeros(32, dtype=np.uint8), C.c_size_t()

        def run(shared, count):
            t0 = time.perf_counter()
            for _ in range(count):
                if shared:
                    rc = lib.zk_batch_prove_shared(bc._h, sdata.ctypes.data_as(C.c_void_p), slen, C.byref(got), sstate.ctypes.data_as(C.c_void_p))
                else:
                    rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p))
                if rc:
                    raise zk.ZkError(rc, lib.zk_last_error().decode())
            return time.perf_counter() - t0

        assert bc.prove_shared().check(strict=True) == 0
        assert bc.prove()[M - 1].check(strict=True) == 0
        for shared in (False, True):
            run(shared, warmup)
        times = {False: [], True: []}
        for _ in range(blocks):
            for shared in (False, True):
                times[shared].append(run(shared, per_block) * 1e3 / (per_block * M))
    fri = leaf_hashes(log_n, log_b, K, coset)
    return {"size": (log_n, log_b, lb), "K": K, "coset": coset, "plain_ms": times[False], "shared_ms": times[True], "plain_bytes": plen,
            "shared_bytes": slen / M, "hash_ratio": (1 + fri / M) / (1 + fri)}


def render(rows, build_hash, blocks, per_block, warmup):
    L = ["Shared proof (zk_batch_prove_shared) beside zk_batch_prove, interleaved in one process and build (tools/batch_shared_bench.py)",
         f"build {build_hash}, {Q} query, cap 0, no early stop; blocks {blocks} x {per_block} calls per entry point, warm-up {warmup} calls; one call in flight",
         "ms and bytes are PER STATEMENT; ratio: shared over separate; hashes: the leaf-hash count of DESIGN.md 7g, shared over separate (a count, not a timing)",
         "",
         "  statements x domain  K  leaves  separate ms  [min .. max]            shared ms  [min .. max]           ratio  hashes   separate B   shared B  ratio"]
    for r in rows:
        log_n, log_b, lb = r["size"]
        p, s = r["plain_ms"], r["shared_ms"]
        pm, sm = statistics.median(p), statistics.median(s)
        L.append(f"  {1 << lb:5d} x 2^{log_n + log_b:<2d}         {r['K']}  {'coset ' if r['coset'] else 'single'}  {pm:10.5f}  [{min(p):.5f} .. {max(p):.5f}]  "
                 f"{sm:10.5f}  [{min(s):.5f} .. {max(s):.5f}]  {sm / pm:5.3f}   {r['hash_ratio']:5.3f}   {r['plain_bytes']:10d}  {r['shared_bytes']:9.1f}  "
                 f"{r['shared_bytes'] / r['plain_bytes']:5.3f}")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_shared_bench.txt"))
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
