#!/usr/bin/env python3
"""Challenges in E in the batched prover: ext_log 0 and 1 with 16 queries, measured in ONE process and build.

Per size (the reference's domain 2^13 with 1 024 proofs per batch; domain 2^20 with 64; domain 2^24 with 8) and per setting (K = 1 with
one-value leaves; K = 3 with coset leaves): one BatchContext with the seeds resident, switched between ext off and on by
zk_batch_set_ext outside the timed windows; a switch re-allocates the layers and the gather buffers, so one untimed batch follows every
switch.  One proof per ext value is checked with the strict verifier and compared with the bytes of the timed call before anything is
timed; then a warm-up of both, then blocks of batches INTERLEAVED over ext off and on, so that drift of the machine hits both alike.
A timed window is a run of zk_batch_prove calls, each of which ends with the proofs on the host.  ms per proof is the median over the
blocks, the spread their minimum and maximum; the yardstick of ext on is ext off in the same run.  Proof bytes are
zk_proof_data_len_ext's.  One batch in flight at a time.  The one-call ext prover (Context(ext_log=1), trace resident) is timed at the
same domain and setting afterwards, one proof at a time.

    python tools/batch_ext_bench.py --out profiles/batch_ext_bench
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
SETTINGS = ((1, False), (3, True))                 # (fold_log, coset_leaves)
EXTS = (0, 1)
Q = 16


def measure_batch(zk, log_n, log_b, log_batch, K, coset, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    batch = 1 << log_batch
    rec = {}
    bufs = {}
    with zk.BatchContext(log_n, log_b, log_batch, queries=Q, fold_log=K, coset_leaves=coset) as bc:
        bc.gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
        for e in EXTS:
            plen = lib.zk_proof_data_len_ext(log_n, log_b, Q, 0, K, int(coset), 0, 0, e)
            bufs[e] = (np.zeros((batch, plen), dtype=np.uint8), np.zeros((batch, 32), dtype=np.uint8), plen)

        def prove(e, count):
            """`count` batches at ext e; returns the seconds of the proving alone (one untimed batch on the new buffers first)."""
            bc.set_ext(e)
            data, states, plen = bufs[e]

            def batches(k):
                for _ in range(k):
                    rc = lib.zk_batch_prove(bc._h, data.ctypes.data_as(C.c_void_p), plen, states.ctypes.data_as(C.c_void_p))
                    if rc:
                        raise zk.ZkError(rc, lib.zk_last_error().decode())

            batches(1)
            t0 = time.perf_counter()
            batches(count)
            return time.perf_counter() - t0

        dev = {}
        for e in EXTS:
            prove(e, 1)
            dev[e] = bc.device_bytes
            p = bc.prove()[batch - 1]
            assert p.ext_log == e and p.check(strict=True) == 0
            assert p.data == bufs[e][0][batch - 1].tobytes()
        for e in EXTS:
            prove(e, warmup)
        times = {e: [] for e in EXTS}
        for _ in range(blocks):
            for e in EXTS:
                times[e].append(prove(e, per_block) * 1e3 / (per_block * batch))
        for e in EXTS:
            t = times[e]
            rec[str(e)] = {"ext_log": e, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                           "proof_bytes": bufs[e][2], "device_bytes": dev[e]}
    return rec


def measure_one_call(zk, log_n, log_b, K, coset, blocks, per_block, warmup):
    """The one-call ext prover on a resident trace: ms per proof, median over the blocks."""
    with zk.Context(log_n, log_b, queries=Q, fold_log=K, coset_leaves=coset, ext_log=1) as ctx:
        ctx.trace_upload(zk.trace_fibsq((1 << log_n) - 1, 1, 3141592))
        assert ctx.prove().check(strict=True) == 0
        for _ in range(warmup):
            ctx.prove()
        t = []
        for _ in range(blocks):
            t0 = time.perf_counter()
            for _ in range(per_block):
                ctx.prove()
            t.append((time.perf_counter() - t0) * 1e3 / per_block)
    return {"ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t}


def render(res):
    L = [f"Challenges in E in the batched prover: ext_log 0 and 1 with {Q} queries, interleaved in one process and build (tools/batch_ext_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} batches per ext value, setting and size, warm-up {res['warmup']} batches; one batch in flight",
         "1/0: ms per proof with ext on over ext off, same run; bytes: zk_proof_data_len_ext; MiB: zk_batch_device_bytes over ext off's",
         "one-call: Context(ext_log=1) on a resident trace at the same domain and setting, ms per proof",
         ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), {1 << rec['log_batch']} proofs per batch (log_batch {rec['log_batch']})")
        L.append("  setting      ext  ms/proof median  [min .. max]            1/0   ranges 1 vs 0      bytes q=16  bytes 1/0     + MiB   one-call ext ms [min .. max]")
        for s in rec["settings"]:
            off = s["ext"]["0"]
            for e in EXTS:
                r = s["ext"][str(e)]
                apart = "-" if not e else ("below, disjoint" if r["ms_max"] < off["ms_min"] else "above, disjoint" if r["ms_min"] > off["ms_max"] else "overlap")
                ratio = f"{r['ms_median'] / off['ms_median']:6.3f}" if e else "     -"
                bratio = f"{r['proof_bytes'] / off['proof_bytes']:6.3f}" if e else "     -"
                oc = s["one_call"]
                one = f"{oc['ms_median']:9.4f} [{oc['ms_min']:.4f} .. {oc['ms_max']:.4f}]" if e else ""
                L.append(f"  K={s['fold_log']} {'coset' if s['coset_leaves'] else 'plain'}    {e}   {r['ms_median']:10.5f}     [{r['ms_min']:.5f} .. {r['ms_max']:.5f}]   {ratio}  {apart:17s}  "
                         f"{r['proof_bytes']:9d}  {bratio}  {(r['device_bytes'] - off['device_bytes']) / 2**20:8.1f}   {one}")
        L.append("")
    if res.get("notes"):
        L.extend(res["notes"])
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_ext_bench"))
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
    sizes = SIZES if args.sizes is None else [SIZES[int(i)] for i in args.sizes.split(",")]
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "notes": args.note, "sizes": []}
    for log_n, log_b, log_batch in sizes:
        rec = {"log_n": log_n, "log_blowup": log_b, "log_batch": log_batch, "domain_log": log_n + log_b, "queries": Q, "settings": []}
        for K, coset in SETTINGS:
            rec["settings"].append({"fold_log": K, "coset_leaves": coset,
                                    "ext": measure_batch(zk, log_n, log_b, log_batch, K, coset, args.blocks, args.per_block, args.warmup),
                                    "one_call": measure_one_call(zk, log_n, log_b, K, coset, args.blocks, args.per_block, args.warmup)})
        res["sizes"].append(rec)
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
