#!/usr/bin/env python3
"""Coset leaves off / on for each folding factor K = 1, 2, 3, measured in ONE process and build (docs/LOG.md).

Per size (domain 2^24, 2^20 and the reference's 2^13): one context per (K, coset) with the trace resident, a warm-up, then blocks
of 20 proofs INTERLEAVED over the six settings (K1 off, K1 on, K2 off, ...), so that drift of the machine hits every setting
alike; ms per proof is the median over the blocks, the spread their minimum and maximum.  The yardstick of a coset-on column is
the coset-off column of the same K and run.  Then, untimed, one proof per setting with every kernel class bracketed
(zk_kernel_stats), and the new kernel alone: zk_merkle_commit_coset of a random layer of the full domain with only the leaf class
bracketed (that class then holds coset_leaf_hash_kernel and nothing else), against the hash-issue floor bench.py's HASH_MODEL
gives for one leaf hash per 2^steps values.

    python tools/coset_leaf_bench.py --out profiles/coset_leaf_bench
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
SETTINGS = [(K, on) for K in KS for on in (False, True)]


def key(K, on):
    return f"K{K}_{'on' if on else 'off'}"


def proof_bytes(zk, log_n, log_b, q, K, on):
    fn = zk.load().zk_proof_data_len_coset if on else zk.load().zk_proof_data_len_fold
    return fn(log_n, log_b, q, 0, K)


def measure_size(zk, log_n, log_b, blocks, per_block, warmup):
    trace = zk.trace_fibsq((1 << log_n) - 1)
    ctxs = {}
    rec = {"log_n": log_n, "log_blowup": log_b, "domain_log": log_n + log_b, "settings": {}}
    try:
        for K, on in SETTINGS:
            ctxs[K, on] = zk.Context(log_n, log_b, fold_log=K, coset_leaves=on)
            ctxs[K, on].trace_upload(trace)
        for s in SETTINGS:
            for _ in range(warmup):
                p = ctxs[s].prove()
            assert p.check(strict=True) == 0
        times = {s: [] for s in SETTINGS}
        for _ in range(blocks):
            for s in SETTINGS:
                t0 = time.perf_counter()
                for _ in range(per_block):
                    ctxs[s].prove()
                times[s].append((time.perf_counter() - t0) * 1e3 / per_block)
        for K, on in SETTINGS:
            c = ctxs[K, on]
            c.set_profiling("all")
            c.kernel_stats(reset=True)
            c.prove()
            ks = c.kernel_stats(reset=True)
            c.set_profiling(())
            t = times[K, on]
            merkle = {k: ks[k] for k in ("merkle_leaf", "merkle_inner", "merkle_top")}
            rec["settings"][key(K, on)] = {
                "K": K, "coset": on, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                "proof_bytes_q1": proof_bytes(zk, log_n, log_b, 1, K, on), "proof_bytes_q32": proof_bytes(zk, log_n, log_b, 32, K, on),
                "merkle": merkle, "merkle_ms": sum(m["ms"] for m in merkle.values()), "merkle_ops": sum(m["ops"] for m in merkle.values()),
                "merkle_launches": sum(m["launches"] for m in merkle.values()), "fold": ks["fri_fold"], "compose": ks["compose"],
                "kernel_ms_total": sum(v["ms"] for v in ks.values())}
    finally:
        for c in ctxs.values():
            c.close()
    return rec


def leaf_kernel_alone(zk, log_n, log_b, reps=20):
    """coset_leaf_hash_kernel by itself on a layer of the full domain, per hash and steps.  The layer (64 MiB at 2^24) stays in the
    last-level cache between the repetitions; the kernel is bound by hash issue, not by its 4 bytes per value."""
    import numpy as np
    from bench_legs import HASH_MODEL, mix_peak_tops
    out = {}
    for hash_name in ("sha256", "field"):
        with zk.Context(log_n, log_b, hash=hash_name) as c:
            c.layer_write(1, np.random.default_rng(1).integers(0, 3221225473, 1 << (log_n + log_b), dtype=np.uint32))
            for steps in (1, 2, 3):
                for _ in range(3):
                    c.merkle_commit(1, coset_steps=steps)
                c.sync()
                c.set_profiling(("merkle_leaf",))
                c.kernel_stats(reset=True)
                for _ in range(reps):
                    c.merkle_commit(1, coset_steps=steps)
                c.sync()
                f = c.kernel_stats(reset=True)["merkle_leaf"]
                c.set_profiling(())
                leaves = 1 << (log_n + log_b - steps)
                ms = f["ms"] / f["launches"]
                floor_ms = leaves * HASH_MODEL[hash_name]["leaf_ops"] / (mix_peak_tops(hash_name) * 1e12) * 1e3
                out[f"{hash_name}_steps{steps}"] = {"hash": hash_name, "steps": steps, "launches": f["launches"], "ms_per_launch": ms, "leaves": leaves,
                                                    "leaf_hashes_per_s": leaves / (ms * 1e-3), "bytes_per_launch": f["bytes"] / f["launches"],
                                                    "issue_floor_ms": floor_ms, "floor_over_measured": floor_ms / ms}
    return out


def render(res):
    L = ["Coset leaves off / on, K = 1, 2, 3, interleaved in one process and build (tools/coset_leaf_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} proofs per setting and size, warm-up {res['warmup']}", ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), SHA-256")
        L.append("  K  coset   ms/proof median  [min .. max]      on/off   ranges        bytes q=1   bytes q=32   merkle launches / ms      kernels ms")
        for K in KS:
            off, on = rec["settings"][key(K, False)], rec["settings"][key(K, True)]
            verdict = "on below off" if on["ms_max"] < off["ms_min"] else "off below on" if off["ms_max"] < on["ms_min"] else "overlap"
            for r in (off, on):
                L.append(f"  {K}  {'on ' if r['coset'] else 'off'}   {r['ms_median']:10.4f}     [{r['ms_min']:.4f} .. {r['ms_max']:.4f}]   "
                         f"{(r['ms_median'] / off['ms_median']):6.3f}   {(verdict if r['coset'] else ''):12s}  {r['proof_bytes_q1']:9d}  {r['proof_bytes_q32']:11d}   "
                         f"{r['merkle_launches']:4d} / {r['merkle_ms']:8.4f}          {r['kernel_ms_total']:8.4f}")
        L.append("")
    if res.get("leaf_kernel"):
        L.append(f"coset_leaf_hash_kernel alone, layer of 2^{res['leaf_kernel_log_m']} values (cache-warm: the same layer every repetition); floor = leaves x")
        L.append("HASH_MODEL leaf_ops at the mix-weighted issue peak of the nominal clock (bench_legs.mix_peak_tops)")
        for f in res["leaf_kernel"].values():
            L.append(f"  {f['hash']:6s} steps {f['steps']}: {f['ms_per_launch']:.4f} ms per launch, {f['leaf_hashes_per_s'] / 1e9:.3f} G leaf hashes/s; "
                     f"issue floor {f['issue_floor_ms']:.4f} ms = {f['floor_over_measured']:.2f} of the measured time")
        L.append("")
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coset_leaf_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "sizes": []}
    for log_n, log_b in SIZES:
        res["sizes"].append(measure_size(zk, log_n, log_b, args.blocks, args.per_block, args.warmup))
        print(f"domain 2^{log_n + log_b} done", flush=True)
    res["leaf_kernel_log_m"] = 24
    res["leaf_kernel"] = leaf_kernel_alone(zk, 21, 3)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
