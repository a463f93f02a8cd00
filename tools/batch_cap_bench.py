#!/usr/bin/env python3
"""Merkle caps in the batched prover: cap_log c = 0, 4, 8 with 16 queries (K = 1, one-value leaves), measured in ONE process and build
(DESIGN.md 7f "Caps in the batched prover").

Per size (the reference's domain 2^13 with 1 024 proofs per batch; domain 2^20 with 64; domain 2^24 with 8): one BatchContext with the
seeds resident, switched between the caps by zk_batch_set_merkle_cap outside the timed windows; a switch re-allocates the gather
buffers and, where the cap lies deeper in the batch heap than the mailbox holds (1 024 x 2^13 at c = 4 and 8, 64 x 2^20 and 8 x 2^24 at c = 8), the
pinned buffer its digests are posted to, so one untimed batch follows every switch.  One proof per cap is checked with the strict
verifier and compared with the bytes of the timed call before anything is timed; then a warm-up of every cap, then blocks of batches
INTERLEAVED over the caps, so that drift of the machine hits every one alike.  A timed window is a run of zk_batch_prove calls, each
of which ends with the proofs on the host.  ms per proof is the median over the blocks, the spread their minimum and maximum; the
yardstick of a c > 0 is c = 0 in the same run.  Proof bytes are zk_proof_data_len_cap's.  One batch in flight at a time.

The split of a batch's commit phase -- the time zk_batch_prove waits for the device and the time its host threads hash cap commits --
comes from the ZK_HOST_TIMING laps of the library, which are read once per process: a child process of this tool, started before
this one touches the GPU, runs every size and cap with the laps on and this one reads its stderr (median of --lap-reps batches).

    python tools/batch_cap_bench.py --out profiles/batch_cap_bench
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((10, 3, 10), (17, 3, 6), (21, 3, 3))      # (log_n, log_blowup, log_batch)
CAPS = (0, 4, 8)
Q = 16


def measure_size(zk, log_n, log_b, log_batch, blocks, per_block, warmup):
    import numpy as np
    lib = zk.load()
    batch = 1 << log_batch
    rec = {"log_n": log_n, "log_blowup": log_b, "log_batch": log_batch, "domain_log": log_n + log_b, "queries": Q, "caps": {}}
    bufs = {}
    with zk.BatchContext(log_n, log_b, log_batch, queries=Q) as bc:
        bc.gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
        for c in CAPS:
            plen = lib.zk_proof_data_len_cap(log_n, log_b, Q, 0, 1, 0, 0, c)
            bufs[c] = (np.zeros((batch, plen), dtype=np.uint8), np.zeros((batch, 32), dtype=np.uint8), plen)

        def prove(c, count):
            """`count` batches at cap c; returns the seconds of the proving alone (one untimed batch on the new buffers first)."""
            bc.set_merkle_cap(c)
            data, states, plen = bufs[c]

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
        for c in CAPS:
            prove(c, 1)
            dev[c] = bc.device_bytes
            p = bc.prove()[batch - 1]
            assert p.cap_log == c and p.check(strict=True) == 0
            assert p.data == bufs[c][0][batch - 1].tobytes()
        for c in CAPS:
            prove(c, warmup)
        times = {c: [] for c in CAPS}
        for _ in range(blocks):
            for c in CAPS:
                times[c].append(prove(c, per_block) * 1e3 / (per_block * batch))
        for c in CAPS:
            t = times[c]
            rec["caps"][str(c)] = {"cap_log": c, "ms_median": statistics.median(t), "ms_min": min(t), "ms_max": max(t), "ms_blocks": t,
                                   "proof_bytes": bufs[c][2], "device_bytes": dev[c]}
    return rec


def laps_child(sizes, reps):
    """Runs in a process of its own with ZK_HOST_TIMING set: per size and cap a marker line on stderr, then `reps` batches."""
    import zkstark_amd as zk
    for i, (log_n, log_b, log_batch) in enumerate(sizes):
        batch = 1 << log_batch
        with zk.BatchContext(log_n, log_b, log_batch, queries=Q) as bc:
            bc.gen_fibsq([1] * batch, [3141592 + p for p in range(batch)])
            for c in CAPS:
                bc.set_merkle_cap(c)
                bc.prove_raw()
                bc.prove_raw()
                for _ in range(reps):
                    print(f"[cap bench] size {i} cap {c}", file=sys.stderr, flush=True)
                    bc.prove_raw()
                    print("[cap bench] end", file=sys.stderr, flush=True)   # the laps of the unmarked batches belong to nobody


def read_laps(text, n_sizes):
    """{(size, cap): {"commit_phase_us", "wait_us", "cap_hash_us"}}: medians over the marked batches."""
    got, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"\[cap bench\] size (\d+) cap (\d+)", line)
        if m:
            cur = got.setdefault((int(m.group(1)), int(m.group(2))), {"commit_phase_us": [], "wait_us": [], "cap_hash_us": []})
            continue
        if line.startswith("[cap bench] end"):
            cur = None
        if cur is None:
            continue
        for name, pat in (("commit_phase_us", r"lde \.\. last roots\s+([0-9.]+) us"), ("wait_us", r"waiting for the device ([0-9.]+) us"),
                          ("cap_hash_us", r"hashing cap commits ([0-9.]+) us")):
            m = re.search(pat, line)
            if m:
                cur[name].append(float(m.group(1)))
    return {k: {n: (statistics.median(v) if v else 0.0) for n, v in d.items()} for k, d in got.items()}


def render(res):
    L = [f"Merkle caps in the batched prover: c = 0, 4, 8 with {Q} queries (K = 1, one-value leaves), interleaved in one process and build (tools/batch_cap_bench.py)",
         f"build {res['build_hash']}, blocks {res['blocks']} x {res['per_block']} batches per cap and size, warm-up {res['warmup']} batches; one batch in flight",
         "c/0: ms per proof at that c over ms per proof at c = 0, same run; bytes: zk_proof_data_len_cap; pinned: device_bytes over c = 0's",
         "per batch, from a run of its own with ZK_HOST_TIMING: commit phase (lde .. last roots), of which the call waits for the device and its host threads hash cap commits",
         ""]
    for rec in res["sizes"]:
        L.append(f"domain 2^{rec['domain_log']} (log_n {rec['log_n']}, log_blowup {rec['log_blowup']}), {1 << rec['log_batch']} proofs per batch (log_batch {rec['log_batch']})")
        L.append("  c  ms/proof median  [min .. max]            c/0   ranges c vs 0      bytes q=16  bytes c/0  pinned KiB   commit ms   wait ms  cap hash ms")
        off = rec["caps"]["0"]
        for c in CAPS:
            r = rec["caps"][str(c)]
            apart = "-" if not c else ("below, disjoint" if r["ms_max"] < off["ms_min"] else "above, disjoint" if r["ms_min"] > off["ms_max"] else "overlap")
            ratio = f"{r['ms_median'] / off['ms_median']:6.3f}" if c else "     -"
            bratio = f"{r['proof_bytes'] / off['proof_bytes']:6.3f}" if c else "     -"
            lp = r.get("laps")
            laps = f"{lp['commit_phase_us'] / 1e3:9.3f} {lp['wait_us'] / 1e3:9.3f} {lp['cap_hash_us'] / 1e3:11.3f}" if lp else "        -         -           -"
            L.append(f"  {c}  {r['ms_median']:10.5f}     [{r['ms_min']:.5f} .. {r['ms_max']:.5f}]   {ratio}  {apart:17s}  {r['proof_bytes']:9d}  {bratio}  "
                     f"{(r['device_bytes'] - off['device_bytes']) / 1024:10.0f}   {laps}")
        L.append("")
    if res.get("notes"):
        L.extend(res["notes"])
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_cap_bench"))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--per-block", type=int, default=4, help="batches per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lap-reps", type=int, default=5)
    ap.add_argument("--sizes", default=None, help="comma-separated indices into the three sizes (default: all)")
    ap.add_argument("--note", action="append", default=[], help="a line appended to the .txt")
    ap.add_argument("--from-json", default=None, help="measure nothing: write the .txt again from this .json of an earlier run")
    ap.add_argument("--laps-child", action="store_true", help=argparse.SUPPRESS)
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
    if args.laps_child:
        laps_child(sizes, args.lap_reps)
        return
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--laps-child", "--lap-reps", str(args.lap_reps)]
                           + (["--sizes", args.sizes] if args.sizes else []), env=dict(os.environ, ZK_HOST_TIMING="1"),
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    if child.returncode:
        sys.stderr.write(child.stderr[-4000:])
        raise SystemExit(f"the laps run failed ({child.returncode}): nothing is measured after a failed GPU process")
    laps = read_laps(child.stderr, len(sizes))
    import zkstark_amd as zk
    from zkstark_amd import _lib
    res = {"build_hash": _lib.build_hash(), "blocks": args.blocks, "per_block": args.per_block, "warmup": args.warmup, "lap_reps": args.lap_reps,
           "notes": args.note, "sizes": []}
    for i, (log_n, log_b, log_batch) in enumerate(sizes):
        rec = measure_size(zk, log_n, log_b, log_batch, args.blocks, args.per_block, args.warmup)
        for c in CAPS:
            if (i, c) in laps:
                rec["caps"][str(c)]["laps"] = laps[i, c]
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
