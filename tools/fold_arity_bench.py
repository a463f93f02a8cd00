#!/usr/bin/env python3
"""FRI folding factor 2^K, K = 1, 2, 3, measured in ONE process and build (DESIGN.md "Folding factor"; docs/LOG.md).

Per size (domain 2^24, 2^20 and the reference's 2^13): one context per K with the trace resident, a warm-up, then blocks of 20
proofs INTERLEAVED over K (1, 2, 3, 1, 2, 3, ...), so that drift of the machine hits every factor alike; ms per proof is the
median over the blocks, the spread their minimum and maximum.  Then, untimed, one proof per K with every kernel class bracketed:
launches, ms and algorithmic bytes of the fold and Merkle classes (zk_kernel_stats).  The yardstick for K = 2, 3 is K = 1 of the
same run; --parent-ms / --this-ms record what `python bench.py` printed for the parent commit and for this one on the same
machine, for the .txt.

    python tools/fold_arity_bench.py --out profiles/fold_arity_bench
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((21, 3), (17, 3), (10, 3))
KS = (1, 2, 3)
HBM_PEAK = 8.0e12            # bytes / s
FOLD_K1_FRACTION = 0.42      # the stand-alone factor-2 fold (README)


def groups(log_n, K):
    return [(r0, min(K, log_n - r0)) for r0 in range(0, log_n, K)]


def measure_size(zk, log_n, log_b, blocks, per_block, warmup):
    trace = zk.trace_fibsq((1 << log_n) - 1)
    ctxs = {}
    for K in KS:
        ctxs[K] = zk.Context(log_n, log_b, fold_log=K)
        ctxs[K].trace_upload(trace)
    rec = {"log_n": log_n, "log_blowup": log_b, "domain_log": log_n + log_b, "per_k": {}}
    try:
        for K in KS:
            for _ in range(warmup):
                p = ctxs[K].prove()
            assert p.check(strict=True) == 0
        times = {K: [] for K in KS}
        for _ in range(blocks):
            for K in KS:
                t0 = time.perf_counter()
                for _ in range(per_block):
                    ctxs[K].prove()
                times[K].append((time.perf_counter() - t0) * 1e3 / per_block)
        for K in KS:
            c = ctxs[K]
            c.set_profiling("all")
            c.kernel_stats(reset=True)
            c.prove()
            ks = c.kernel_stats(reset=True)
            c.set_profiling(())
            fold = ks["fri_fold"]
            merkle = {k: ks[k] for k in ("merkle_leaf", "merkle_inner", "merkle_top")}
            trees = 2 + len(groups(log_n, K))
            r = {"ms_median": statistics.median(times[K]), "ms_min": min(times[K]), "ms_max": max(times[K]), "ms_blocks": times[K],
                 "proof_bytes_q1": zk.load().zk_proof_data_len_fold(log_n, log_b, 1, 0, K),
                 "proof_bytes_q32": zk.load().zk_proof_data_len_fold(log_n, log_b, 32, 0, K),
                 "trees": trees, "host_round_trips": trees + 1,           # one per commitment, one for the decommitment fetch
                 "fold": fold, "merkle": merkle, "merkle_ms": sum(m["ms"] for m in merkle.values()),
                 "merkle_launches": sum(m["launches"] for m in merkle.values()), "kernel_ms_total": sum(v["ms"] for v in ks.values())}
            if fold["launches"] and fold["ms"] > 0:
                r["fold_bytes_per_s"] = fold["bytes"] / (fold["ms"] * 1e-3)
                r["fold_fraction_of_hbm_peak"] = r["fold_bytes_per_s"] / HBM_PEAK
            rec["per_k"][str(K)] = r
    finally:
        for c in ctxs.values():
            c.close()
    return rec


def fold_kernel_alone(zk, log_n, log_b, reps=20):
    """The multi-fold launch of the first group by itself (layer 1 -> layer 1 + steps at the full domain), timed with events.  The
    input (64 MiB at 2^24) stays in the last-level cache between the repetitions: a cache-warm rate, not HBM bandwidth."""
    import numpy as np
    out = {}
    with zk.Context(log_n, log_b) as c:
        rng = np.random.default_rng(1)
        c.layer_write(1, rng.integers(0, 3221225473, 1 << (log_n + log_b), dtype=np.uint32))
        for steps in (1, 2, 3):
            for _ in range(3):
                c.fri_fold_multi(0, steps, 12345)
            c.sync()
            c.set_profiling(("fri_fold",))
            c.kernel_stats(reset=True)
            for _ in range(reps):
                c.fri_fold_multi(0, steps, 12345)
            c.sync()
            f = c.kernel_stats(reset=True)["fri_fold"]
            c.set_profiling(())
            bps = f["bytes"] / (f["ms"] * 1e-3)
            out[str(steps)] = {"launches": f["launches"], "ms_per_launch": f["ms"] / f["launches"], "bytes_per_launch": f["bytes"] / f["launches"],
                               "bytes_per_s": bps, "fraction_of_hbm_peak": bps / HBM_PEAK}
    return out


def render(res):
    L = ["FRI folding factor 2^K: K = 1, 2, 3 interleaved in one process and build (tools/fold_arity_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} proofs per K and size, warm-up {res['warmup']}", ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']})")
        L.append("  K   ms/proof median  [min .. max]     vs K=1   trees  round trips  bytes q=1   bytes q=32   fold launches/ms    merkle launches/ms")
        base = rec["per_k"]["1"]["ms_median"]
        for K in KS:
            r = rec["per_k"][str(K)]
            L.append(f"  {K}   {r['ms_median']:10.4f}     [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]   {r['ms_median'] / base:6.3f}   {r['trees']:5d}  {r['host_round_trips']:11d}"
                     f"  {r['proof_bytes_q1']:9d}  {r['proof_bytes_q32']:11d}   {r['fold']['launches']:4d} / {r['fold']['ms']:8.4f}     {r['merkle_launches']:4d} / {r['merkle_ms']:8.4f}")
        for K in KS:
            r = rec["per_k"][str(K)]
            if "fold_bytes_per_s" in r:
                L.append(f"  K = {K}: stand-alone fold launches inside a proof: {r['fold']['bytes'] / 1e6:.1f} MB in {r['fold']['ms']:.4f} ms = "
                         f"{r['fold_bytes_per_s'] / 1e12:.2f} TB/s = {100 * r['fold_fraction_of_hbm_peak']:.0f} % of 8 TB/s")
        L.append("")
    if res.get("fold_kernel"):
        L.append(f"multi-fold kernel alone, layer of 2^{res['fold_kernel_log_m']} values (algorithmic bytes 4 m (1 + 2^-steps)); the factor-2 fold is quoted at "
                 f"{100 * FOLD_K1_FRACTION:.0f} % of 8 TB/s")
        L.append("  CAVEAT: the same 64 MiB input is folded over and over, and it fits in the 256 MiB last-level cache, so these are cache-warm")
        L.append("  rates (an upper bound), NOT HBM bandwidth, and not comparable with a figure taken on cold data; steps 1 is the existing")
        L.append("  fri_fold_kernel4, the very kernel the 42 % is quoted for, and it shows the same effect.  Read the three rows against each other.")
        for s, f in res["fold_kernel"].items():
            L.append(f"  steps {s}: {f['ms_per_launch']:.4f} ms, {f['bytes_per_s'] / 1e12:.2f} TB/s = {100 * f['fraction_of_hbm_peak']:.0f} % of 8 TB/s "
                     f"({f['fraction_of_hbm_peak'] / FOLD_K1_FRACTION:.2f} x the 42 %)")
        L.append("")
    L.append("yardsticks (python bench.py, domain 2^24, same machine):")
    L.append(f"  parent commit: {res.get('parent_bench_ms')} ms per proof; this commit: {res.get('this_bench_ms')} ms per proof; "
             f"K = 1 above: {res['sizes'][0]['per_k']['1']['ms_median']:.4f} ms")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fold_arity_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-ms", default=None, help="ms per proof `python bench.py` printed for the parent commit on this machine")
    ap.add_argument("--this-ms", default=None, help="the same for this commit")
    args = ap.parse_args()
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup,
           "parent_bench_ms": args.parent_ms, "this_bench_ms": args.this_ms, "sizes": []}
    for log_n, log_b in SIZES:
        res["sizes"].append(measure_size(zk, log_n, log_b, args.blocks, args.per_block, args.warmup))
        print(f"domain 2^{log_n + log_b} done", flush=True)
    res["fold_kernel_log_m"] = 24
    res["fold_kernel"] = fold_kernel_alone(zk, 21, 3)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
