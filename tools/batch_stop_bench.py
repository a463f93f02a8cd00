#!/usr/bin/env python3
"""Early stop in the batched prover: D = stop_log 0, 4, 8 at (K = 1, one-value leaves) and (K = 3, coset leaves), six configurations
measured in ONE process and build (DESIGN.md 7d "Early stop in the batched prover").

Per size (the reference's domain 2^13 with 1 024 proofs per batch; domain 2^20 with 64; domain 2^24 with 8: the throughput shape
README quotes): one BatchContext with the seeds resident, switched between the configurations by zk_batch_set_fri_stop /
zk_batch_set_fold / zk_batch_set_coset_leaves outside the timed windows; a switch re-allocates the gather buffers and the tables of the
final polynomials, so one untimed batch follows every switch.  One proof per configuration is checked with the strict
verifier and compared with the bytes of the timed call before anything is timed; then a warm-up of every configuration, then blocks
of batches INTERLEAVED over the six configurations, so that drift of the machine hits every one alike.  A timed window is a run of
zk_batch_prove calls, each of which ends with the proofs on the host (a device synchronise inside the call).  ms per proof is the
median over the blocks, the spread their minimum and maximum.  The yardstick of a D > 0 is D = 0 of the same format in the same
run.  Proof bytes are zk_proof_data_len_stop's for one query.  One batch in flight at a time.

    python tools/batch_stop_bench.py --out profiles/batch_stop_bench
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

SIZES = ((10, 3, 10), (17, 3, 6), (21, 3, 3))      # (log_n, log_blowup, log_batch)
STOPS = (0, 4, 8)
FORMATS = ((1, False), (3, True))                  # (fold_log, coset leaves)
CONFIGS = tuple((K, coset, D) for K, coset in FORMATS for D in STOPS)


def key(K, coset, D):
    return f"K{K}_{'coset' if coset else 'plain'}_D{D}"


def measure_size(zk, log_n, log_b, log_batch, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    batch = 1 << log_batch
    rec = {"log_n": log_n, "log_blowup": log_b, "log_batch": log_batch, "domain_log": log_n + log_b, "configs": {}}
    bufs = {}
    with zk.BatchContext(log_n, log_b, log_batch) as bc:
        bc.gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
        for K, coset, D in CONFIGS:
            plen = lib.zk_proof_data_len_stop(log_n, log_b, 1, 0, K, int(coset), D)
            bufs[K, coset, D] = (np.zeros((batch, plen), dtype=np.uint8), np.zeros((batch, 32), dtype=np.uint8), plen)

        def switch(K, coset, D):
            bc.set_fri_stop(0)                              # every intermediate combination is one the limits admit
            bc.set_fold(K)
            bc.set_coset_leaves(coset)
            bc.set_fri_stop(D)

        def prove(K, coset, D, count):
            """`count` batches of one configuration; returns the seconds of the proving alone.  The switch frees and allocates the
            gather buffers and the tables of the final polynomials, so one untimed batch runs on the new buffers first: the timed
            window never touches freshly allocated pinned memory."""
            switch(K, coset, D)
            data, states, plen = bufs[K, coset, D]

            def batches(k):
                for _ in range(k):
                    rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p))
                    if rc:
                        raise zk.ZkError(rc, lib.zk_last_error().decode())

            batches(1)
            t0 = time.perf_counter()
            batches(count)
            return time.perf_counter() - t0

        for K, coset, D in CONFIGS:
            prove(K, coset, D, 1)
            p = bc.prove()[batch - 1]
            assert (p.fold_log, p.coset_leaves, p.stop_log) == (K, coset, D) and p.check(strict=True) == 0
            assert p.data == bufs[K, coset, D][0][batch - 1].tobytes()
        for c in CONFIGS:
            prove(*c, warmup)
        times = {c: [] for c in CONFIGS}
        for _ in range(blocks):
            for c in CONFIGS:
                times[c].append(prove(*c, per_block) * 1e3 / (per_block * batch))
        for K, coset, D in CONFIGS:
            t = times[K, coset, D]
            rec["configs"][key(K, coset, D)] = {"K": K, "coset": coset, "stop_log": D, "ms_median": statistics.median(t), "ms_min": min(t),
                                                "ms_max": max(t), "ms_blocks": t, "proof_bytes_q1": bufs[K, coset, D][2]}
        rec["device_bytes"] = bc.device_bytes
    return rec


def render(res):
    L = ["Early stop in the batched prover: D = 0, 4, 8 x (K = 1 one-value leaves, K = 3 coset leaves), interleaved in one process and build (tools/batch_stop_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} batches per configuration and size, warm-up {res['warmup']} batches; one batch in flight",
         "D/0: ms per proof at that D over ms per proof at D = 0 of the same format, same run; bytes: zk_proof_data_len_stop, one query", ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), {1 << rec['log_batch']} proofs per batch (log_batch {rec['log_batch']})")
        L.append("  K  leaves  D  ms/proof median  [min .. max]            D/0   ranges D vs 0      bytes q=1  bytes D/0")
        for K, coset in FORMATS:
            off = rec["configs"][key(K, coset, 0)]
            for D in STOPS:
                r = rec["configs"][key(K, coset, D)]
                apart = "-" if not D else ("below, disjoint" if r["ms_max"] < off["ms_min"] else "above, disjoint" if r["ms_min"] > off["ms_max"] else "overlap")
                ratio = f"{r['ms_median'] / off['ms_median']:6.3f}" if D else "     -"
                bratio = f"{r['proof_bytes_q1'] / off['proof_bytes_q1']:6.3f}" if D else "     -"
                L.append(f"  {K}  {'coset' if coset else 'plain'}   {D}  {r['ms_median']:10.5f}     [{r['ms_min']:.5f} .. {r['ms_max']:.5f}]   {ratio}  {apart:17s}  {r['proof_bytes_q1']:9d}  {bratio}")
        L.append("")
    if res.get("notes"):
        L.extend(res["notes"])
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_stop_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4, help="batches per block")
    ap.add_argument("--warmup", type=int, default=2)
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
