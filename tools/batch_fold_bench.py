#!/usr/bin/env python3
"""FRI folding factor 2^K in the batched prover, K = 1, 2, 3, measured in ONE process and build (DESIGN.md "Folding factor").

Per size (domain 2^24 with 8 proofs per batch: the throughput shape README quotes; domain 2^20 with 64; the reference's 2^13 with
1 024): one BatchContext per K with the seeds resident, a warm-up, then blocks of batches INTERLEAVED over K (1, 2, 3, 1, 2, 3,
...), so that drift of the machine hits every factor alike; ms per proof is the median over the blocks, the spread their minimum
and maximum.  One proof per K is checked with the strict verifier before anything is timed.  The yardstick for K = 2, 3 is K = 1
of the same run (the default path, which zk_batch_set_fold does not touch); --parent-ms / --this-ms record what `python bench.py`
printed for the parent commit and for this one on the same machine, for the .txt.  One batch in flight at a time; two in flight
is tools/batch_inflight.py's subject.

    python tools/batch_fold_bench.py --out profiles/batch_fold_bench
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((21, 3, 3), (17, 3, 6), (10, 3, 10))      # (log_n, log_blowup, log_batch)
KS = (1, 2, 3)


def groups(log_n, K):
    return [(r0, min(K, log_n - r0)) for r0 in range(0, log_n, K)]


def hashed_leaves(log_n, log_b, K):
    """Leaves under the trees of one proof: f, cp and one layer per group."""
    N = 1 << (log_n + log_b)
    return 2 * N + sum(N >> (r0 + s) for r0, s in groups(log_n, K))


def measure_size(zk, log_n, log_b, log_batch, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    batch = 1 << log_batch
    rec = {"log_n": log_n, "log_blowup": log_b, "log_batch": log_batch, "domain_log": log_n + log_b, "per_k": {}}
    ctxs, bufs = {}, {}
    try:
        for K in KS:
            ctxs[K] = zk.BatchContext(log_n, log_b, log_batch, fold_log=K)
            ctxs[K].gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
            plen = lib.zk_proof_data_len_fold(log_n, log_b, 1, 0, K)
            bufs[K] = (np.zeros((batch, plen), dtype=np.uint8), np.zeros((batch, 32), dtype=np.uint8), plen)

        def prove(K):
            data, states, plen = bufs[K]
            rc = lib.zk_batch_prove(ctxs[K]._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p))
            if rc:
                raise zk.ZkError(rc, lib.zk_last_error().decode())

        for K in KS:
            for _ in range(warmup):
                prove(K)
            p = ctxs[K].prove()[batch - 1]
            assert p.fold_log == K and p.check(strict=True) == 0
            assert p.data == bufs[K][0][batch - 1].tobytes()
        times = {K: [] for K in KS}
        for _ in range(blocks):
            for K in KS:
                t0 = time.perf_counter()
                for _ in range(per_block):
                    prove(K)
                times[K].append((time.perf_counter() - t0) * 1e3 / (per_block * batch))
        for K in KS:
            rec["per_k"][str(K)] = {"ms_median": statistics.median(times[K]), "ms_min": min(times[K]), "ms_max": max(times[K]), "ms_blocks": times[K],
                                    "proof_bytes_q1": bufs[K][2], "trees": 2 + len(groups(log_n, K)),
                                    "hashed_leaves": hashed_leaves(log_n, log_b, K), "device_bytes": ctxs[K].device_bytes}
    finally:
        for c in ctxs.values():
            c.close()
    return rec


def render(res):
    L = ["FRI folding factor 2^K in the batched prover: K = 1, 2, 3 interleaved in one process and build (tools/batch_fold_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} batches per K and size, warm-up {res['warmup']} batches; one batch in flight", ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), {1 << rec['log_batch']} proofs per batch (log_batch {rec['log_batch']})")
        L.append("  K   ms/proof median  [min .. max]       vs K=1   ranges vs K=1   trees  leaves hashed vs K=1  bytes q=1   device GiB")
        base = rec["per_k"]["1"]
        for K in KS:
            r = rec["per_k"][str(K)]
            apart = "-" if K == 1 else ("below, disjoint" if r["ms_max"] < base["ms_min"] else "above, disjoint" if r["ms_min"] > base["ms_max"] else "overlap")
            L.append(f"  {K}   {r['ms_median']:10.5f}     [{r['ms_min']:.5f} .. {r['ms_max']:.5f}]   {r['ms_median'] / base['ms_median']:6.3f}   {apart:15s} {r['trees']:5d}"
                     f"  {r['hashed_leaves'] / base['hashed_leaves']:20.3f}  {r['proof_bytes_q1']:9d}   {r['device_bytes'] / 2**30:10.2f}")
        L.append("")
    L.append("yardsticks (python bench.py, one proof at a time, domain 2^24, same machine):")
    L.append(f"  parent commit: {res.get('parent_bench_ms')} ms per proof; this commit: {res.get('this_bench_ms')} ms per proof")
    if res.get("notes"):
        L.append("")
        L.extend(res["notes"])
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_fold_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=8, help="batches per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-ms", default=None, help="ms per proof `python bench.py` printed for the parent commit on this machine")
    ap.add_argument("--this-ms", default=None, help="the same for this commit")
    ap.add_argument("--note", action="append", default=[], help="a line appended to the .txt (e.g. a tools/batch_inflight.py figure)")
    ap.add_argument("--from-json", default=None, help="measure nothing: write the .txt again from this .json of an earlier run")
    args = ap.parse_args()
    if args.from_json:
        with open(args.from_json) as f:
            res = json.load(f)
        res["notes"] = res.get("notes", []) + args.note
        with open(args.out + ".txt", "w") as f:
            f.write(render(res))
        print(render(res))
        return
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup,
           "parent_bench_ms": args.parent_ms, "this_bench_ms": args.this_ms, "notes": args.note, "sizes": []}
    for log_n, log_b, log_batch in SIZES:
        res["sizes"].append(measure_size(zk, log_n, log_b, log_batch, args.blocks, args.per_block, args.warmup))
        print(f"domain 2^{log_n + log_b} x {1 << log_batch} done", flush=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
