#!/usr/bin/env python3
"""SHA-256 against BLAKE2s-256 as the Merkle hash of the one-call prover: time per proof and the rate of the compiled
inner hash, in one process.

Three settings, one context each, at the domains 2^13, 2^20 and 2^24 (log_n = 10, 17, 21 with blow-up 8):

    sha256            SHA-256 with the default host levels: the headline setting (the host hashes the tree tops and the FRI tail)
    sha256_device     SHA-256 with host levels (0, 0): every tree on the device, as every BLAKE2s tree is
    blake2s           BLAKE2s-256 (always on the device)

The timed proofs are taken round-robin -- one proof of each setting per round, --rounds rounds after --warmup untimed ones -- so that
drift of the machine falls on every setting alike.  A proof is Context.prove() on a resident trace: the call returns when the proof
bytes are on the host, so the host clock around it measures the whole proof.  Per setting: median, minimum and maximum over the
rounds, and the medians' ratio to `sha256`.  Every setting's first proof is checked with the CPU verifier (strict) before anything
is timed.  Then zk_probe_hash_chain for both hashes at 1, 2 and 4 waves per SIMD: nanoseconds per inner hash per SIMD, the floor a
tree kernel can reach.

    python tools/hash_kinds_bench.py [--rounds 15] [--warmup 3] [--domains 13,20,24] [--out profiles/hash_kinds_bench.txt]

Needs a GPU; fails without one.  Writes a text table (and one JSON line at its end) to --out and to stdout.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zkstark_amd as zk  # noqa: E402

LOG_B = 3
SETTINGS = (("sha256", "sha256", None), ("sha256_device", "sha256", (0, 0)), ("blake2s", "blake2s", None))


def bench_domain(log_domain, rounds, warmup):
    log_n = log_domain - LOG_B
    trace = zk.trace_fibsq((1 << log_n) - 1, 1, 3141592)
    ctxs = []
    try:
        for name, hash_name, levels in SETTINGS:
            ctx = zk.Context(log_n, LOG_B, hash=hash_name, host_levels=levels)
            ctx.trace_upload(trace)
            ctx.prove().verify(strict=True)                      # also the first warm-up: code objects loaded, buffers touched
            ctxs.append((name, ctx))
        times = {name: [] for name, _ in ctxs}
        for r in range(warmup + rounds):
            for name, ctx in ctxs:
                t0 = time.perf_counter()
                ctx.prove()
                dt = time.perf_counter() - t0
                if r >= warmup:
                    times[name].append(dt * 1e6)
    finally:
        for _, ctx in ctxs:
            ctx.close()
    out = {}
    for name, ts in times.items():
        out[name] = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "proofs": len(ts)}
    for name in out:
        out[name]["ratio_to_sha256"] = out[name]["median_us"] / out["sha256"]["median_us"]
    return out


def bench_probe():
    out = {}
    for hash_name in ("sha256", "blake2s"):
        for waves in (1, 2, 4):
            r = zk.probe_hash_chain(hash_name, waves_per_simd=waves, hashes=64, launches=20)
            out[f"{hash_name}_w{waves}"] = {"ns_per_hash_per_simd": r["ns_per_hash_per_simd"], "clock_ghz": r["clock_ghz"]}
    for waves in (1, 2, 4):
        out[f"ratio_w{waves}"] = out[f"blake2s_w{waves}"]["ns_per_hash_per_simd"] / out[f"sha256_w{waves}"]["ns_per_hash_per_simd"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--domains", default="13,20,24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_kinds_bench.txt"))
    a = ap.parse_args()
    res = {"rounds": a.rounds, "warmup": a.warmup, "log_b": LOG_B, "domains": {}}
    lines = [f"hash_kinds_bench: {a.rounds} timed rounds after {a.warmup} warm-up rounds, settings interleaved per round, blow-up 2^{LOG_B}", ""]
    for d in [int(x) for x in a.domains.split(",")]:
        r = res["domains"][str(d)] = bench_domain(d, a.rounds, a.warmup)
        lines.append(f"domain 2^{d} (log_n {d - LOG_B}): microseconds per proof")
        for name, _, _ in SETTINGS:
            v = r[name]
            lines.append(f"  {name:14s} median {v['median_us']:10.1f}   min {v['min_us']:10.1f}   max {v['max_us']:10.1f}   x {v['ratio_to_sha256']:.3f} of sha256")
        lines.append("")
    p = res["probe"] = bench_probe()
    lines.append("zk_probe_hash_chain: ns per inner hash per SIMD (64 hashes per lane, 20 launches)")
    for waves in (1, 2, 4):
        lines.append(f"  {waves} wave(s) per SIMD: sha256 {p[f'sha256_w{waves}']['ns_per_hash_per_simd']:8.1f}   blake2s {p[f'blake2s_w{waves}']['ns_per_hash_per_simd']:8.1f}"
                     f"   x {p[f'ratio_w{waves}']:.3f}   (clock {p[f'blake2s_w{waves}']['clock_ghz']:.2f} GHz)")
    lines += ["", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
