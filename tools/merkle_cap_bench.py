#!/usr/bin/env python3
"""Merkle caps, cap_log c = 0, 4, 8, measured in ONE process and build (docs/LOG.md).

Per size (domain 2^13 -- the reference's --, 2^20 and 2^24), per configuration ((K = 1, one-value leaves, D = 0) and (K = 3, coset
leaves, D = 6)) and per host-levels setting (the default, and off = zk_ctx_set_host_levels(0, 0)): one context with the trace
resident and 32 queries, a warm-up of every c, then blocks of proofs INTERLEAVED round-robin over c (0, 4, 8, 0, 4, ...;
zk_ctx_set_merkle_cap between the blocks), so that drift of the machine hits every setting alike.  ms per proof is the median over the
blocks, the range their minimum and maximum; the proof length (zk_proof_data_len_cap) is printed beside it.  The yardstick is c = 0 of
the same run, configuration and host levels, which is the code path of a build without the option.  Two settings differ only when
their ranges do not overlap.  A record, not a gate: nothing here has a threshold.

    python tools/merkle_cap_bench.py --out profiles/merkle_cap_bench [--sizes 10,17,21]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((10, 3), (17, 3), (21, 3))
CONFIGS = ((1, False, 0), (3, True, 6))              # (fold_log, coset leaves, stop_log)
CAPS = (0, 4, 8)
QUERIES = 32


def measure(zk, log_n, log_b, K, coset, D, levels, blocks, per_block, warmup):
    lib = zk.load()
    rec = {"fold_log": K, "coset_leaves": coset, "stop_log": D, "host_levels": "default" if levels is None else "off", "per_cap": {}}
    with zk.Context(log_n, log_b, queries=QUERIES, fold_log=K, coset_leaves=coset, stop_log=D, host_levels=levels) as ctx:
        ctx.trace_upload(zk.trace_fibsq((1 << log_n) - 1))
        for c in CAPS:
            ctx.set_merkle_cap(c)
            for _ in range(warmup):
                p = ctx.prove()
            assert p.check(strict=True) == 0, (log_n, K, coset, D, c)
        times = {c: [] for c in CAPS}
        for _ in range(blocks):
            for c in CAPS:
                ctx.set_merkle_cap(c)
                t0 = time.perf_counter()
                for _ in range(per_block):
                    ctx.prove()                           # returns with the proof bytes on the host: the device is idle again
                times[c].append((time.perf_counter() - t0) * 1e3 / per_block)
        for c in CAPS:
            t = times[c]
            rec["per_cap"][str(c)] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                                      "proof_bytes": lib.zk_proof_data_len_cap(log_n, log_b, QUERIES, 0, K, int(coset), D, c)}
    return rec


def render(res):
    L = ["Merkle caps: cap_log c = 0, 4, 8 interleaved round-robin in one process and build (tools/merkle_cap_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} proofs per setting, warm-up {res['warmup']}; {QUERIES} queries, no grinding",
         "c = 0 is the code path of a build without the option; 'differs' = the [min .. max] ranges of c and c = 0 do not overlap", ""]
    for size in res["sizes"]:
        L.append(f"domain 2^{size['domain_log']} (log_n {size['log_n']}, log_blowup {size['log_blowup']})")
        for rec in size["configs"]:
            L.append(f"  K = {rec['fold_log']}, {'coset' if rec['coset_leaves'] else 'one-value'} leaves, D = {rec['stop_log']}, host levels {rec['host_levels']}")
            L.append("    c   ms/proof median  [min .. max]      vs c=0   differs   proof bytes")
            base = rec["per_cap"]["0"]
            for c in CAPS:
                r = rec["per_cap"][str(c)]
                apart = "-" if c == 0 else ("yes" if r["ms_max"] < base["ms_min"] or r["ms_min"] > base["ms_max"] else "no")
                L.append(f"    {c}   {r['ms_median']:10.4f}     [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]   {r['ms_median'] / base['ms_median']:6.3f}   {apart:>7}   {r['proof_bytes']:11d}")
        L.append("")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_cap_bench"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="", help="log_n of the sizes to run, e.g. 10,17 (default: all three)")
    args = ap.parse_args()
    import zkstark_amd as zk
    from zkstark_amd import _lib
    want = {int(v) for v in args.sizes.split(",")} if args.sizes else None
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "caps": list(CAPS),
           "queries": QUERIES, "sizes": []}
    for log_n, log_b in SIZES:
        if want is not None and log_n not in want:
            continue
        size = {"log_n": log_n, "log_blowup": log_b, "domain_log": log_n + log_b, "configs": []}
        for K, coset, D in CONFIGS:
            for levels in (None, (0, 0)):
                size["configs"].append(measure(zk, log_n, log_b, K, coset, D, levels, args.blocks, args.per_block, args.warmup))
        res["sizes"].append(size)
        print(f"domain 2^{log_n + log_b} done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
