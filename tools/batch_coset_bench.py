#!/usr/bin/env python3
"""Coset leaves in the batched prover: K = 1, 2, 3 with one-value leaves and with coset leaves, six configurations measured in ONE
process and build.

Per size (domain 2^24 with 8 proofs per batch: the throughput shape README quotes; domain 2^20 with 64; the reference's 2^13 with
1 024): one BatchContext per K with the seeds resident, switched between the two leaf formats by zk_batch_set_coset_leaves outside
the timed windows (six resident batches of 2^24 x 8 would take 150 GiB).  One proof per configuration is checked with the strict
verifier before anything is timed; then a warm-up of every configuration, then blocks of batches INTERLEAVED over the six
configurations, so that drift of the machine hits every one alike.  ms per proof is the median over the blocks, the spread their
minimum and maximum.  The yardstick of "coset on" at a K is "coset off" at the same K in the same run.  Next to the measured
ratio stands the ratio of hashed leaves (f, cp and one layer per group; a coset leaf counts once), which is what the time would
follow if hashing were all of it.  One batch in flight at a time.

    python tools/batch_coset_bench.py --out profiles/batch_coset_bench
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
CONFIGS = tuple((K, coset) for K in KS for coset in (False, True))


def groups(log_n, K):
    return [(r0, min(K, log_n - r0)) for r0 in range(0, log_n, K)]


def hashed_leaves(log_n, log_b, K, coset):
    """Leaves under the trees of one proof: f, cp and one layer per group; with coset leaves the tree over a group's input layer has
    one leaf per coset of that group (f and the last layer keep one-value leaves)."""
    N = 1 << (log_n + log_b)
    grp = groups(log_n, K)
    if not coset:
        return 2 * N + sum(N >> (r0 + s) for r0, s in grp)
    return N + sum((N >> r0) >> s for r0, s in grp) + (N >> log_n)


def key(K, coset):
    return f"K{K}_{'coset' if coset else 'plain'}"


def measure_size(zk, log_n, log_b, log_batch, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    batch = 1 << log_batch
    rec = {"log_n": log_n, "log_blowup": log_b, "log_batch": log_batch, "domain_log": log_n + log_b, "configs": {}}
    ctxs, bufs = {}, {}
    try:
        for K in KS:
            ctxs[K] = zk.BatchContext(log_n, log_b, log_batch, fold_log=K)
            ctxs[K].gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
        for K, coset in CONFIGS:
            plen = (lib.zk_proof_data_len_coset if coset else lib.zk_proof_data_len_fold)(log_n, log_b, 1, 0, K)
            bufs[K, coset] = (np.zeros((batch, plen), dtype=np.uint8), np.zeros((batch, 32), dtype=np.uint8), plen)

        def prove(K, coset, count):
            """`count` batches of configuration (K, coset); returns the seconds of the proving alone (the switch is outside)."""
            ctxs[K].set_coset_leaves(coset)
            data, states, plen = bufs[K, coset]
            t0 = time.perf_counter()
            for _ in range(count):
                rc = lib.zk_batch_prove(ctxs[K]._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p))
                if rc:
                    raise zk.ZkError(rc, lib.zk_last_error().decode())
            return time.perf_counter() - t0

        for K, coset in CONFIGS:
            prove(K, coset, 1)
            p = ctxs[K].prove()[batch - 1]
            assert p.fold_log == K and p.coset_leaves == coset and p.check(strict=True) == 0
            assert p.data == bufs[K, coset][0][batch - 1].tobytes()
        for K, coset in CONFIGS:
            prove(K, coset, warmup)
        times = {c: [] for c in CONFIGS}
        for _ in range(blocks):
            for K, coset in CONFIGS:
                times[K, coset].append(prove(K, coset, per_block) * 1e3 / (per_block * batch))
        for K, coset in CONFIGS:
            t = times[K, coset]
            rec["configs"][key(K, coset)] = {"K": K, "coset": coset, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                                             "proof_bytes_q1": bufs[K, coset][2], "hashed_leaves": hashed_leaves(log_n, log_b, K, coset),
                                             "device_bytes": ctxs[K].device_bytes}
    finally:
        for c in ctxs.values():
            c.close()
    return rec


def render(res):
    L = ["Coset leaves in the batched prover: K = 1, 2, 3 x (one-value leaves, coset leaves), interleaved in one process and build (tools/batch_coset_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} batches per configuration and size, warm-up {res['warmup']} batches; one batch in flight",
         "on/off: ms per proof with coset leaves over ms per proof with one-value leaves at the same K; leaves on/off: the same ratio of hashed leaves", ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), {1 << rec['log_batch']} proofs per batch (log_batch {rec['log_batch']})")
        L.append("  K  leaves  ms/proof median  [min .. max]          on/off  ranges on vs off   leaves on/off  leaves hashed / N  bytes q=1")
        N = 1 << rec["domain_log"]
        for K in KS:
            off = rec["configs"][key(K, False)]
            for coset in (False, True):
                r = rec["configs"][key(K, coset)]
                apart = "-" if not coset else ("below, disjoint" if r["ms_max"] < off["ms_min"] else "above, disjoint" if r["ms_min"] > off["ms_max"] else "overlap")
                ratio = f"{r['ms_median'] / off['ms_median']:6.3f}" if coset else "     -"
                lratio = f"{r['hashed_leaves'] / off['hashed_leaves']:6.3f}" if coset else "     -"
                L.append(f"  {K}  {'coset' if coset else 'plain'}   {r['ms_median']:10.5f}     [{r['ms_min']:.5f} .. {r['ms_max']:.5f}]   {ratio}  {apart:17s}  {lratio}"
                         f"        {r['hashed_leaves'] / N:12.3f}      {r['proof_bytes_q1']:9d}")
        L.append("")
    if res.get("notes"):
        L.extend(res["notes"])
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_coset_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=8, help="batches per block")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default=None, help="comma-separated indices into the three sizes (default: all)")
    ap.add_argument("--note", action="append", default=[], help="a line appended to the .txt")
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
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "notes": args.note, "sizes": []}
    sizes = SIZES if args.sizes is None else [SIZES[int(i)] for i in args.sizes.split(",")]
    for log_n, log_b, log_batch in sizes:
        res["sizes"].append(measure_size(zk, log_n, log_b, log_batch, args.blocks, args.per_block, args.warmup))
        print(f"domain 2^{log_n + log_b} x {1 << log_batch} done", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1)
    txt = render(res)
    with open(args.out + ".txt", "w") as f:
        f.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
