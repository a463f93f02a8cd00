#!/usr/bin/env python3
"""Early stop of FRI, stop_log D = 0, 2, 4, 6, 8, measured in ONE process and build (DESIGN.md 7d "Early stop"; docs/LOG.md).

Per size (domain 2^13 -- the reference's --, 2^20 and 2^24) and per configuration ((K = 1, one-value leaves), (K = 3, one-value
leaves), (K = 3, coset leaves)): one context with the trace resident, a warm-up of every D, then blocks of proofs INTERLEAVED
round-robin over D (0, 2, 4, 6, 8, 0, 2, ...; zk_ctx_set_fri_stop between the blocks), so that drift of the machine hits every
setting alike.  ms per proof is the median over the blocks, the range their minimum and maximum; the proof length of each setting
is printed beside it.  The yardstick is D = 0 of the same run and configuration, which is the code path of a build without the
option.  Two settings differ only when their ranges do not overlap.

    python tools/fri_stop_bench.py --out profiles/fri_stop_bench
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
CONFIGS = ((1, False), (3, False), (3, True))        # (fold_log, coset leaves)
STOPS = (0, 2, 4, 6, 8)


def measure(zk, log_n, log_b, K, coset, blocks, per_block, warmup):
    lib = zk.load()
    rec = {"fold_log": K, "coset_leaves": coset, "per_stop": {}}
    with zk.Context(log_n, log_b, fold_log=K, coset_leaves=coset) as ctx:
        ctx.trace_upload(zk.trace_fibsq((1 << log_n) - 1))
        for D in STOPS:
            ctx.set_fri_stop(D)
            for _ in range(warmup):
                p = ctx.prove()
            assert p.check(strict=True) == 0, (log_n, K, coset, D)
        times = {D: [] for D in STOPS}
        for _ in range(blocks):
            for D in STOPS:
                ctx.set_fri_stop(D)
                t0 = time.perf_counter()
                for _ in range(per_block):
                    ctx.prove()                           # returns with the proof bytes on the host: the device is idle again
                times[D].append((time.perf_counter() - t0) * 1e3 / per_block)
        for D in STOPS:
            t = times[D]
            rec["per_stop"][str(D)] = {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                                       "proof_bytes_q1": lib.zk_proof_data_len_stop(log_n, log_b, 1, 0, K, int(coset), D),
                                       "proof_bytes_q32": lib.zk_proof_data_len_stop(log_n, log_b, 32, 0, K, int(coset), D),
                                       "groups": -(-(log_n - D) // K)}
    return rec


def render(res):
    L = ["Early stop of FRI: stop_log D = 0, 2, 4, 6, 8 interleaved round-robin in one process and build (tools/fri_stop_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} proofs per setting, warm-up {res['warmup']}; one query, no grinding",
         "D = 0 is the code path of a build without the option; 'differs' = the [min .. max] ranges of D and D = 0 do not overlap", ""]
    for size in res["sizes"]:
        L.append(f"domain 2^{size['domain_log']} (log_n {size['log_n']}, log_blowup {size['log_blowup']})")
        for rec in size["configs"]:
            L.append(f"  K = {rec['fold_log']}, {'coset' if rec['coset_leaves'] else 'one-value'} leaves")
            L.append("    D   groups   ms/proof median  [min .. max]      vs D=0   differs   bytes q=1   bytes q=32")
            base = rec["per_stop"]["0"]
            for D in STOPS:
                r = rec["per_stop"][str(D)]
                apart = "-" if D == 0 else ("yes" if r["ms_max"] < base["ms_min"] or r["ms_min"] > base["ms_max"] else "no")
                L.append(f"    {D}   {r['groups']:6d}   {r['ms_median']:10.4f}     [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]   {r['ms_median'] / base['ms_median']:6.3f}   {apart:>7}"
                         f"   {r['proof_bytes_q1']:9d}   {r['proof_bytes_q32']:10d}")
        L.append("")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_stop_bench"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "stops": list(STOPS),
           "sizes": []}
    for log_n, log_b in SIZES:
        size = {"log_n": log_n, "log_blowup": log_b, "domain_log": log_n + log_b, "configs": []}
        for K, coset in CONFIGS:
            size["configs"].append(measure(zk, log_n, log_b, K, coset, args.blocks, args.per_block, args.warmup))
        res["sizes"].append(size)
        print(f"domain 2^{log_n + log_b} done", flush=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
