#!/usr/bin/env python3
"""Proof-of-work grinding on one MI355X (DESIGN.md "Grinding"): search rates and what grinding adds to a proof.

    python tools/grind_bench.py [--out FILE.json] [--quick]

* search: zk_grind (device) and zk_grind_host at 1 and 16 threads, several random states per g.  The rate is the nonces a
  search had to test (the smallest nonce + 1) over its wall time (each call ends with its result on the host);
  median and spread over the states, and the mean nonces per search against the expected 2^g;
* small g: device and one host thread side by side (the provers' host / device threshold, kGrindHostMaxBits);
* per proof: zk_prove at domains 2^20 and 2^24 with g = 16, 20, 24 against g = 0, alternating inside this process;
* batch: zk_batch_prove of 8 proofs at 2^20 with g = 20 against g = 0, per proof.
Prints one line per row and, with --out, the whole record as JSON.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import zkstark_amd as zk  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, time.perf_counter() - t


def search_rows(rng, quick):
    rows = []
    plan = {16: 8, 20: 8, 24: 6, 28: 3, 32: 2} if not quick else {16: 3, 20: 3, 24: 2}
    for g, states in plan.items():
        sts = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(states)]
        row = {"g": g, "states": states, "expected_nonces": 2 ** g}
        for who, fn, max_g in (("device", lambda s: zk.grind(s, g), 32), ("host16", lambda s: zk.grind_host(s, g, 0, 16), 28),
                               ("host1", lambda s: zk.grind_host(s, g, 0, 1), 20)):
            if g > max_g:
                continue
            rates, tested = [], []
            for s in sts[: (2 if who == "host16" and g >= 28 else states)]:
                w, dt = timed(lambda: fn(s))
                rates.append((w + 1) / dt)
                tested.append(w + 1)
            row[who] = {"nonces_per_s_median": statistics.median(rates), "min": min(rates), "max": max(rates),
                        "mean_nonces_per_search": statistics.mean(tested)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def small_g_rows(rng):
    rows = []
    for g in (6, 8, 10, 12, 14, 16, 18):
        sts = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(16)]
        dev = [timed(lambda: zk.grind(s, g))[1] * 1e6 for s in sts]
        host = [timed(lambda: zk.grind_host(s, g, 0, 1))[1] * 1e6 for s in sts]
        row = {"g": g, "device_us_median": statistics.median(dev), "host1_us_median": statistics.median(host)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def proof_rows(quick):
    rows = []
    for log_n in ((17, 21) if not quick else (17,)):
        trace = zk.trace_fibsq((1 << log_n) - 1)
        reps = 8 if log_n == 17 else 5
        for g in (16, 20, 24):
            with zk.Context(log_n, 3) as c0, zk.Context(log_n, 3, grind_bits=g) as cg:
                c0.trace_upload(trace)
                cg.trace_upload(trace)
                c0.prove()
                cg.prove()
                t0, tg = [], []
                for _ in range(reps):                          # alternating: both see the same machine state
                    t0.append(timed(c0.prove)[1] * 1e3)
                    tg.append(timed(cg.prove)[1] * 1e3)
            row = {"domain_log": log_n + 3, "g": g, "ms_g0_median": statistics.median(t0), "ms_g_median": statistics.median(tg),
                   "added_ms_median": statistics.median(tg) - statistics.median(t0), "ms_g0_all": t0, "ms_g_all": tg}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def batch_row():
    log_n, lb = 17, 3
    a1s = [3141592 + p for p in range(1 << lb)]
    out = {}
    with zk.BatchContext(log_n, 3, lb) as b0, zk.BatchContext(log_n, 3, lb, grind_bits=20) as bg:
        for b in (b0, bg):
            b.gen_fibsq([1] * len(a1s), a1s)
            b.prove_raw()
        t0, tg = [], []
        for _ in range(5):
            t0.append(timed(b0.prove_raw)[1] * 1e3 / len(a1s))
            tg.append(timed(bg.prove_raw)[1] * 1e3 / len(a1s))
    out = {"batch": len(a1s), "domain_log": log_n + 3, "g": 20, "ms_per_proof_g0_median": statistics.median(t0),
           "ms_per_proof_g_median": statistics.median(tg), "added_ms_per_proof": statistics.median(tg) - statistics.median(t0)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--part", choices=("all", "search", "prove"), default="all")
    a = ap.parse_args()
    zk.load()
    rng = random.Random(2026)
    rec = {"build_hash": zk._lib.build_hash(), "host_hash_mode": zk.host_hash_mode()}
    zk.grind(bytes(32), 12)                                # first launch: code object load
    if a.part in ("all", "search"):
        rec["search"] = search_rows(rng, a.quick)
        rec["small_g"] = small_g_rows(rng)
    if a.part in ("all", "prove"):
        rec["proof"] = proof_rows(a.quick)
        rec["batch"] = batch_row()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
