"""Batched GPU verification against the CPU verifier: one JSON line.

For each shape: the wall time of zk_verifier_run (Verifier.verify_raw: warm-up, then --steps timed calls, each ending in the
call's own synchronisation), and the CPU's time for the same proofs with zk_verify_queries on 1 thread and on a 16-thread
pool (ctypes releases the GIL).  --profile adds per-kernel times from a separate `rocprofv3 --kernel-trace --stats` run per
shape (this script again with --inner).  Not part of bench.py: it measures this one feature.

--fold K[,K...] measures proofs with the FRI folding factor 2^K (BatchContext(fold_log=K), Verifier(fold_log=K); the CPU side
is zk_verify_fold).  With several K the timed calls are taken in --blocks rounds that visit every K in turn, in this one
process, so that drift of the machine falls on every K alike; a result is then named NAME_kK and carries the median, minimum
and maximum over all its calls.

--coset measures every K of --fold twice, with coset leaves off and on (Verifier(coset_leaves=True)), the two interleaved in the
same rounds.  The coset proofs come from the one-call prover (Context(coset_leaves=True); the batch prover has no coset leaves), the
CPU side of a coset column is zk_verify_coset; a coset result is named NAME_kK_coset.

--stop D0,D1,... measures every K and leaf format of the other options once per listed D (Verifier(stop_log=D); 0 = proofs folded
down to a constant), all interleaved in the same rounds.  The stopped proofs come from the one-call prover (Context(stop_log=D)), the
CPU side is zk_verify_stop, and every distinct proof is first checked with zk_verify_stop (strict) before it is timed; a result is
named NAME_kK[_coset]_dD.

--cap C0,C1,... measures every setting of the other options once per listed cap_log (Verifier(cap_log=c); 0 = roots), all interleaved in
the same rounds.  The capped proofs come from the one-call prover (Context(cap_log=c)), the CPU side is zk_verify_cap, every distinct
proof is first checked with it (strict), and proof_bytes is zk_proof_data_len_cap; a result is named NAME_kK[_coset][_dD]_cC.

--shared LB[,LB...] [--rows] measures shared proofs of 2^LB statements each (Verifier(log_batch=LB, shared_rows=--rows)) over the shapes
of SHARED_SHAPES: K = 1 with one-value leaves and K = 3 with coset leaves, the query counts of --queries (1 and 16, the most the batched
prover makes), strict.  The proofs come from
BatchContext.prove_shared (two distinct ones per setting, tiled), each checked with zk_verify_shared_rows (strict) before it is timed.  The
yardstick is zk_verify_shared_rows on a 16-thread pool in this process: per setting, --blocks rounds of --steps GPU calls and one pass
of the pool, in turn, so that drift falls on both alike; both are reported as medians, a result is named NAME_lbLB[_rows]_kK[_coset]_qQ.
A shape whose batch does not fit the device is reported with its error.

--ext [E0,E1] measures proofs over E (Verifier(ext_log=1)) beside base-field proofs (bare --ext: 0,1) on 1 024 proofs of 2^13, 1 024 at
domain 2^20 and 16 at 2^24: K = 1 with one-value leaves and K = 3 with coset leaves, q = 1, SHA-256, strict.  The proofs come from the
one-call prover (Context(ext_log=E), a few distinct ones per setting, tiled), each checked on the CPU before it is timed.  Per setting one
verifier per ext_log lives in the same process: --blocks rounds of --steps GPU calls per ext_log in turn, then one pass of a 16-thread
pool per ext_log over the same proofs (zk_verify_ext; with ext_log 0 that is zk_verify_cap).  Medians; a result is named
NAME_COUNT_kK[_coset]_extE.  --ext 0 measures the base-field side alone, the run to compare two builds by.

    python tools/verify_bench.py [--steps 20] [--warmup 3] [--profile] [--only NAME,...] [--fold 1,2,3 --blocks 5] [--coset] [--stop 0,4,8] [--cap 0,4,8]
    python tools/verify_bench.py --ext [0,1] [--steps 20] [--blocks 3] [--only 2e13_1024,2e20_64,2e24_16]
    python tools/verify_bench.py --shared 3,6 [--rows] [--queries 1,16] [--steps 3 --blocks 3] [--only NAME,...]
"""
import argparse
import concurrent.futures
import csv
import ctypes as C
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zkstark_amd as zk  # noqa: E402
from zkstark_amd import _lib  # noqa: E402

# name: (log_n, log_b, queries, hash, count, strict); proofs come from the batch prover, tiled when the count exceeds what one
# batch of that size proves cheaply (the verifier does not care that two proofs are equal)
SHAPES = {
    "ref_strict_1024": (10, 3, 1, "sha256", 1024, True),
    "ref_plain_1024": (10, 3, 1, "sha256", 1024, False),
    "2e20_strict_1024": (17, 3, 1, "sha256", 1024, True),
    "2e24_q1_strict_16": (21, 3, 1, "sha256", 16, True),
    "2e24_q16_strict_16": (21, 3, 16, "sha256", 16, True),
    "ref_field_strict_1024": (10, 3, 1, "field", 1024, True),
    "2e24_q1_strict_1": (21, 3, 1, "sha256", 1, True),
    "2e24_q1_strict_8": (21, 3, 1, "sha256", 8, True),
    "2e24_q1_strict_64": (21, 3, 1, "sha256", 64, True),
}
# --shared: name: (log_n, log_b, count)
SHARED_SHAPES = {"2e13_1024": (10, 3, 1024), "2e20_64": (17, 3, 64), "2e24_16": (21, 3, 16)}
PROFILED = ["ref_strict_1024", "ref_plain_1024", "2e20_strict_1024", "2e24_q1_strict_16", "2e24_q16_strict_16", "ref_field_strict_1024"]
_cache = {}
_checked = set()


def proofs_for(log_n, log_b, q, hash, count, fold=1, coset=False, stop=None, cap=None):
    """(data [count, len] uint8, states [count, 32], public_last [count]) of valid proofs.  stop: None, or D of --stop (every distinct
    proof is then checked with zk_verify_stop on the CPU, strict, before anything is timed)."""
    key = (log_n, log_b, q, hash, fold, coset, stop or 0, cap or 0)
    if key not in _cache and (coset or stop or cap):  # the one-call prover, one trace at a time
        with zk.Context(log_n, log_b, hash=hash, queries=q, fold_log=fold, coset_leaves=coset, stop_log=stop or 0, cap_log=cap or 0) as ctx:
            ps = [ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, 3141592 + p)) for p in range(64 if log_n <= 10 else (8 if log_n <= 17 else 2))]
        _cache[key] = (np.stack([np.frombuffer(p.data, dtype=np.uint8) for p in ps]), np.stack([np.frombuffer(p.state, dtype=np.uint8) for p in ps]),
                       np.array([p.public_last & 0xFFFFFFFF for p in ps], dtype=np.uint32))
    if key not in _cache:
        log_batch = 10 if log_n <= 10 else (6 if log_n <= 17 else 1)
        with zk.BatchContext(log_n, log_b, log_batch, hash=hash, queries=q, fold_log=fold) as bc:
            bc.gen_fibsq([1] * bc.batch, [3141592 + p for p in range(bc.batch)])
            data, states = bc.prove_raw()
            _cache[key] = (data, states, bc.public_last())
    if (stop is not None or cap is not None) and key not in _checked:
        data, states, last = _cache[key]
        check = C.c_int32(1)
        for i in range(len(data)):
            rc = _lib.load().zk_verify_cap(data[i].ctypes.data, data.shape[1], states[i].ctypes.data, log_n, log_b, int(last[i]), zk.host.HASHES[hash], q, 0,
                                           fold, int(coset), stop or 0, cap or 0, C.byref(check))
            assert rc == 0 and check.value == 0, (key, i, rc, check.value)
        _checked.add(key)
    data, states, last = _cache[key]
    idx = np.arange(count) % len(data)
    return np.ascontiguousarray(data[idx]), np.ascontiguousarray(states[idx]), np.ascontiguousarray(last[idx])


def gpu_times(shape, steps, warmup, folds=(1,), blocks=1):
    """{K: [ms of every timed call]}: `blocks` rounds over the K of `folds`, `steps` calls each, one verifier per K.  An element
    of folds is K, (K, coset) to choose the leaf format, or (K, coset, D) for proofs stopped at 2^D coefficients (--stop)."""
    log_n, log_b, q, hash, count, strict = shape
    vs, ts = {}, {K: [] for K in folds}
    try:
        for K in folds:
            fold, coset, stop, cap = (K + (None, None))[:4] if isinstance(K, tuple) else (K, False, None, None)
            data, states, last = proofs_for(log_n, log_b, q, hash, count, fold, coset, stop, cap)
            vs[K] = (zk.Verifier(log_n, log_b, hash=hash, queries=q, fold_log=fold, coset_leaves=coset, stop_log=stop or 0, cap_log=cap or 0), data,
                     states if strict else None, last)
            for _ in range(warmup):
                assert (vs[K][0].verify_raw(data, last, vs[K][2]) == 0).all()
        for _ in range(blocks):
            for K in folds:
                v, data, states, last = vs[K]
                for _ in range(steps):
                    t0 = time.perf_counter()
                    v.verify_raw(data, last, states)
                    ts[K].append((time.perf_counter() - t0) * 1e3)
    finally:
        for v in vs.values():
            v[0].close()
    return ts


def cpu_ms(shape, threads, fold=1, coset=False, stop=None, cap=None):
    log_n, log_b, q, hash, count, strict = shape
    data, states, last = proofs_for(log_n, log_b, q, hash, count, fold, coset, stop, cap)
    lib = _lib.load()
    hk = zk.host.HASHES[hash]
    plen = data.shape[1]
    rows = [(data[i].ctypes.data, states[i].ctypes.data if strict else None, int(last[i])) for i in range(count)]
    check = C.c_int32 * 1

    def one(r):
        if cap is not None:
            return lib.zk_verify_cap(r[0], plen, r[1], log_n, log_b, r[2], hk, q, 0, fold, int(coset), stop or 0, cap, check())
        if stop is not None:
            return lib.zk_verify_stop(r[0], plen, r[1], log_n, log_b, r[2], hk, q, 0, fold, int(coset), stop, check())
        if coset:
            return lib.zk_verify_coset(r[0], plen, r[1], log_n, log_b, r[2], hk, q, 0, fold, check())
        if fold != 1:
            return lib.zk_verify_fold(r[0], plen, r[1], log_n, log_b, r[2], hk, q, 0, fold, check())
        return lib.zk_verify_queries(r[0], plen, r[1], log_n, log_b, r[2], hk, q)

    if threads == 1:
        one(rows[0])
        t0 = time.perf_counter()
        rcs = [one(r) for r in rows]
    else:
        with concurrent.futures.ThreadPoolExecutor(threads) as ex:
            list(ex.map(one, rows[:threads]))
            t0 = time.perf_counter()
            rcs = list(ex.map(one, rows, chunksize=max(1, count // (4 * threads))))
    ms = (time.perf_counter() - t0) * 1e3
    assert all(rc == 0 for rc in rcs)
    return ms


def profile(name, steps):
    """Per-kernel totals (ms per zk_verifier_run call) from rocprofv3 --kernel-trace --stats over this script with --inner."""
    rp = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out = tempfile.mkdtemp(prefix="verify_bench_")
    cmd = [rp, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "vb", "--", sys.executable, os.path.abspath(__file__), "--inner", name,
           "--steps", str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
    stats = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                m = re.search(r"(verify_\w+_kernel(?:<\d+>)?)", row.get("Name", ""))
                if m:                                 # --inner makes one warm-up call and `steps` timed ones
                    stats[m.group(1)] = round(stats.get(m.group(1), 0.0) + float(row["TotalDurationNs"]) / 1e6 / (steps + 1), 4)
    shutil.rmtree(out, ignore_errors=True)
    return stats


def shared_result(log_n, log_b, count, lb, rows, K, coset, q, steps, warmup, blocks):
    """One --shared setting: GPU calls and 16-thread CPU passes over the same `count` proofs, in turn."""
    lib = _lib.load()
    kw = dict(queries=q, fold_log=K, coset_leaves=coset)
    with zk.BatchContext(log_n, log_b, log_batch=lb, shared_rows=rows, **kw) as bc:
        ps = []
        for r in range(2):
            bc.gen_fibsq([1] * bc.batch, [3141592 + r * bc.batch + p for p in range(bc.batch)])
            ps.append(bc.prove_shared())
    for p in ps:
        assert p.check(strict=True) == 0
    idx = np.arange(count) % len(ps)
    data = np.ascontiguousarray(np.stack([np.frombuffer(p.data, dtype=np.uint8) for p in ps])[idx])
    states = np.ascontiguousarray(np.stack([np.frombuffer(p.state, dtype=np.uint8) for p in ps])[idx])
    last = np.ascontiguousarray(np.stack([np.asarray(p.public_last, dtype=np.uint32) for p in ps])[idx])
    plen = data.shape[1]
    jobs = [(data[i].ctypes.data, states[i].ctypes.data, last[i].ctypes.data) for i in range(count)]
    check = C.c_int32 * 1

    def one(r):
        return lib.zk_verify_shared_rows(r[0], plen, r[1], log_n, log_b, r[2], lb, 0, q, 0, K, int(coset), 0, 0, int(rows), check())

    gpu, cpu = [], []
    with zk.Verifier(log_n, log_b, log_batch=lb, shared_rows=rows, **kw) as v, concurrent.futures.ThreadPoolExecutor(16) as ex:
        assert v.proof_len == plen
        for _ in range(warmup):
            assert (v.verify_raw(data, last, states) == 0).all()
        list(ex.map(one, jobs[:16]))
        for _ in range(blocks):
            for _ in range(steps):
                t0 = time.perf_counter()
                v.verify_raw(data, last, states)
                gpu.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            rcs = list(ex.map(one, jobs, chunksize=max(1, count // 64)))
            cpu.append((time.perf_counter() - t0) * 1e3)
            assert all(rc == 0 for rc in rcs)
    gpu.sort()
    cpu.sort()
    return {"log_n": log_n, "log_blowup": log_b, "count": count, "log_batch": lb, "shared_rows": rows, "fold_log": K, "coset_leaves": coset, "queries": q,
            "strict": True, "proof_bytes": plen, "gpu_ms_median": round(gpu[len(gpu) // 2], 4), "gpu_ms_min": round(gpu[0], 4), "gpu_ms_max": round(gpu[-1], 4),
            "cpu_16t_ms_median": round(cpu[len(cpu) // 2], 3), "cpu_16t_ms_min": round(cpu[0], 3),
            "speedup_vs_16t": round(cpu[len(cpu) // 2] / gpu[len(gpu) // 2], 2)}


def shared_main(a):
    lbs = tuple(int(x) for x in a.shared.split(","))
    res = {}
    for name, (log_n, log_b, count) in SHARED_SHAPES.items():
        if a.only and name not in a.only.split(","):
            continue
        for lb in lbs:
            for K, coset in ((1, False), (3, True)):
                for q in (int(x) for x in a.queries.split(",")):
                    key = f"{name}_lb{lb}" + ("_rows" if a.rows else "") + f"_k{K}" + ("_coset" if coset else "") + f"_q{q}"
                    try:
                        res[key] = shared_result(log_n, log_b, count, lb, a.rows, K, coset, q, a.steps, a.warmup, a.blocks)
                    except (zk.ZkError, MemoryError) as e:
                        res[key] = {"error": str(e)[:200]}
                    print(f"# {key}: {res[key]}", file=sys.stderr, flush=True)
    print(json.dumps({"tool": "verify_bench", "build_hash": _lib.build_hash(), "steps": a.steps, "warmup": a.warmup, "blocks": a.blocks, "shared": list(lbs),
                      "rows": a.rows, "shapes": res}), flush=True)


def ext_result(log_n, log_b, count, K, coset, exts, steps, warmup, blocks):
    """One --ext setting: per ext_log of `exts` a verifier and `count` strict SHA-256 proofs with q = 1 from the one-call prover (a few
    distinct ones, tiled).  Every block times `steps` GPU calls per ext_log, in turn, then one pass of the 16-thread pool per ext_log over
    the same proofs (zk_verify_ext; ext_log = 0 is zk_verify_cap, which is what is called, so the mode also runs on a build without ext)."""
    lib = _lib.load()
    kw = dict(queries=1, fold_log=K, coset_leaves=coset)
    check = C.c_int32 * 1
    runs = {}
    for e in exts:
        xkw = dict(kw, ext_log=1) if e else kw
        with zk.Context(log_n, log_b, **xkw) as ctx:
            ps = [ctx.prove(zk.trace_fibsq((1 << log_n) - 1, 1, 3141592 + p)) for p in range(16 if log_n <= 10 else (4 if log_n <= 17 else 2))]
        for p in ps:
            assert p.check(strict=True) == 0
        idx = np.arange(count) % len(ps)
        data = np.ascontiguousarray(np.stack([np.frombuffer(p.data, dtype=np.uint8) for p in ps])[idx])
        states = np.ascontiguousarray(np.stack([np.frombuffer(p.state, dtype=np.uint8) for p in ps])[idx])
        last = np.ascontiguousarray(np.array([p.public_last & 0xFFFFFFFF for p in ps], dtype=np.uint32)[idx])
        runs[e] = {"v": zk.Verifier(log_n, log_b, **xkw), "data": data, "states": states, "last": last, "gpu": [], "cpu": [],
                   "jobs": [(data[i].ctypes.data, states[i].ctypes.data, int(last[i])) for i in range(count)]}

    def one(e, plen):
        if e:
            return lambda r: lib.zk_verify_ext(r[0], plen, r[1], log_n, log_b, r[2], 0, 1, 0, K, int(coset), 0, 0, 1, check())
        return lambda r: lib.zk_verify_cap(r[0], plen, r[1], log_n, log_b, r[2], 0, 1, 0, K, int(coset), 0, 0, check())

    try:
        with concurrent.futures.ThreadPoolExecutor(16) as ex:
            for e, r in runs.items():
                assert r["v"].proof_len == r["data"].shape[1]
                for _ in range(warmup):
                    assert (r["v"].verify_raw(r["data"], r["last"], r["states"]) == 0).all()
                list(ex.map(one(e, r["data"].shape[1]), r["jobs"][:16]))
            for _ in range(blocks):
                for e, r in runs.items():
                    for _ in range(steps):
                        t0 = time.perf_counter()
                        r["v"].verify_raw(r["data"], r["last"], r["states"])
                        r["gpu"].append((time.perf_counter() - t0) * 1e3)
                for e, r in runs.items():
                    t0 = time.perf_counter()
                    rcs = list(ex.map(one(e, r["data"].shape[1]), r["jobs"], chunksize=max(1, count // 64)))
                    r["cpu"].append((time.perf_counter() - t0) * 1e3)
                    assert all(rc == 0 for rc in rcs)
    finally:
        for r in runs.values():
            r["v"].close()
    out = {}
    for e, r in runs.items():
        gpu, cpu = sorted(r["gpu"]), sorted(r["cpu"])
        out[e] = {"log_n": log_n, "log_blowup": log_b, "count": count, "ext_log": e, "fold_log": K, "coset_leaves": coset, "queries": 1, "strict": True,
                  "proof_bytes": int(r["data"].shape[1]), "gpu_ms_median": round(gpu[len(gpu) // 2], 4), "gpu_ms_min": round(gpu[0], 4),
                  "gpu_ms_max": round(gpu[-1], 4), "cpu_16t_ms_median": round(cpu[len(cpu) // 2], 3), "cpu_16t_ms_min": round(cpu[0], 3),
                  "speedup_vs_16t": round(cpu[len(cpu) // 2] / gpu[len(gpu) // 2], 2)}
    return out


def ext_main(a):
    exts = tuple(int(x) for x in a.ext.split(","))
    res = {}
    for name, (log_n, log_b, count) in SHARED_SHAPES.items():      # 1 024 x 2^13, the batch at domain 2^20, 16 x 2^24
        if a.only and name not in a.only.split(","):
            continue
        for K, coset in ((1, False), (3, True)):
            for e, r in ext_result(log_n, log_b, 1024 if name == "2e20_64" else count, K, coset, exts, a.steps, a.warmup, a.blocks).items():
                key = f"{name.rsplit('_', 1)[0]}_{r['count']}_k{K}" + ("_coset" if coset else "") + f"_ext{e}"
                res[key] = r
                print(f"# {key}: {r}", file=sys.stderr, flush=True)
    print(json.dumps({"tool": "verify_bench", "build_hash": _lib.build_hash(), "steps": a.steps, "warmup": a.warmup, "blocks": a.blocks, "ext": list(exts),
                      "shapes": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--inner", default="")
    ap.add_argument("--fold", default="1", help="folding factors 2^K to measure, e.g. 1,2,3 (interleaved in one process)")
    ap.add_argument("--blocks", type=int, default=1, help="rounds over the K of --fold, each of --steps calls per K")
    ap.add_argument("--coset", action="store_true", help="every K with coset leaves off and on, interleaved")
    ap.add_argument("--stop", default="", help="early-stop D to measure, e.g. 0,4,8: every K and leaf format once per D, interleaved")
    ap.add_argument("--cap", default="", help="Merkle cap_log to measure, e.g. 0,4,8: every other setting once per cap, interleaved")
    ap.add_argument("--shared", default="", help="log_batch of shared proofs to measure, e.g. 3,6 (the shapes of SHARED_SHAPES)")
    ap.add_argument("--rows", action="store_true", help="with --shared: proofs with row leaves")
    ap.add_argument("--queries", default="1,16", help="with --shared: the query counts to measure (the batched prover makes at most 16)")
    ap.add_argument("--ext", nargs="?", const="0,1", default="", help="ext_log values to measure, interleaved in one process (bare --ext: 0,1)")
    a = ap.parse_args()
    if a.ext:
        ext_main(a)
        return
    if a.shared:
        shared_main(a)
        return
    folds = tuple(int(k) for k in a.fold.split(","))
    if a.inner:                                       # under rocprofv3: the timed GPU calls of one shape only
        gpu_times(SHAPES[a.inner], a.steps, 1, ((folds[0], True),) if a.coset else folds[:1])
        return
    stops = tuple(int(d) for d in a.stop.split(",")) if a.stop else (None,)
    caps = tuple(int(c) for c in a.cap.split(",")) if a.cap else (None,)
    settings = tuple((K, on, D, c) for K in folds for on in ((False, True) if a.coset else (False,)) for D in stops for c in caps)
    names = [n for n in SHAPES if not a.only or n in a.only.split(",")]
    res = {}
    for name in names:
        shape = SHAPES[name]
        times = gpu_times(shape, a.steps, a.warmup, settings, a.blocks)
        for K, on, D, cap in settings:
            ts = sorted(times[K, on, D, cap])
            c1 = cpu_ms(shape, 1, K, on, D, cap)
            c16 = cpu_ms(shape, 16, K, on, D, cap)
            key = ((name if folds == (1,) and not a.coset and not a.stop and not a.cap else f"{name}_k{K}") + ("_coset" if on else "")
                   + ("" if D is None else f"_d{D}") + ("" if cap is None else f"_c{cap}"))
            res[key] = {"log_n": shape[0], "log_blowup": shape[1], "queries": shape[2], "hash": shape[3], "count": shape[4],
                        "strict": shape[5], "fold_log": K, "coset_leaves": on, "stop_log": D or 0, "cap_log": cap or 0,
                        "proof_bytes": int(_lib.load().zk_proof_data_len_cap(shape[0], shape[1], shape[2], 0, K, int(on), D or 0, cap or 0)),
                        "gpu_ms_median": round(ts[len(ts) // 2], 4), "gpu_ms_min": round(ts[0], 4), "gpu_ms_max": round(ts[-1], 4),
                        "cpu_1t_ms": round(c1, 3), "cpu_16t_ms": round(c16, 3),
                        "speedup_vs_16t": round(c16 / ts[len(ts) // 2], 2)}
            print(f"# {key}: {res[key]}", file=sys.stderr, flush=True)
    if a.profile:
        for name in names:
            if name in PROFILED and name in res:
                res[name]["kernels_ms_per_call"] = profile(name, 5)
    cross = {n: res[n] for n in ("2e24_q1_strict_1", "2e24_q1_strict_8", "2e24_q1_strict_16", "2e24_q1_strict_64") if n in res}
    line = {"tool": "verify_bench", "build_hash": _lib.build_hash(), "steps": a.steps, "warmup": a.warmup, "fold": list(folds), "coset": a.coset, "stop": [d for d in stops if d is not None], "cap": [c for c in caps if c is not None], "blocks": a.blocks, "shapes": res,
            "crossover_2e24_strict": {n: {"count": r["count"], "gpu_ms": r["gpu_ms_median"], "cpu_16t_ms": r["cpu_16t_ms"]} for n, r in cross.items()}}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
