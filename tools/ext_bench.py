"""What challenges in E = F_P[u] / (u^2 - 5) cost (zk_ctx_set_ext): whole proofs, then the two stages that change.

Proofs.  For each domain size (2^13, 2^20, 2^24 by default, blow-up 8) and each of two settings -- K = 3 with coset leaves, where ext off and
on both take the grouped round loop (the like-for-like pair), and K = 1 with one-value leaves, where ext off keeps the fused leaf launches,
the early launch and the host FRI tail -- one context with ext off and one with ext on prove the same resident trace.  The two are
interleaved in --blocks rounds in this one process, so that drift of the machine falls on both alike; a window is --proofs calls of
zk_prove_resident on the host clock (a call returns with the finished proof: it ends synchronised), after a warm-up of both.  Reported per
proof: the median, minimum and maximum over the rounds, ext / base, and the proof sizes from zk_proof_data_len_ext.  The first ext proof of
every pair is verified strictly before anything is timed.

Kernels.  zk_dev_compose against zk_dev_compose_ext, and zk_dev_fri_fold_multi against zk_dev_fri_fold_multi_ext on layer 0 with 1 and 3
steps, interleaved the same way; a window is --reps launches on one stream between two device events.  Reported per launch, with the bytes
the stage must move by count (f or the layer read once, the output written once; the tables are not counted) and that count over the median.
At 2^13 a launch is shorter than its enqueue, so the figure there is the host's launch rate; and a window launches over the same buffers
again and again, which at every size here fit the 256 MB last-level cache, so no rate in that table is an HBM rate.

Not part of bench.py: it measures this one feature.

    python tools/ext_bench.py [--sizes 13,20,24] [--proofs 20] [--reps 2000] [--blocks 5] [--out profiles/ext_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zkstark_amd as zk  # noqa: E402
from zkstark_amd import _lib  # noqa: E402
from zkstark_amd._lib import check  # noqa: E402

P = 3221225473
LOG_B = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="13,20,24", help="log2 of the domain sizes")
    ap.add_argument("--proofs", type=int, default=20, help="proofs per timed window")
    ap.add_argument("--reps", type=int, default=2000, help="launches per timed window of the kernel table")
    ap.add_argument("--blocks", type=int, default=5, help="rounds; each visits base and ext once")
    ap.add_argument("--out", default=None, help="also write the report here")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ext_bench: no GPU; nothing is measured without one")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    name = torch.cuda.get_device_name(0)
    lines = [f"# tools/ext_bench.py on {name}: ms per proof (zk_prove_resident, SHA-256, 1 query), median [min .. max] of {args.blocks} windows of {args.proofs} proofs",
             f"{'setting':<28}{'domain':>8}{'ext':>5}{'proof bytes':>13}{'median ms':>12}{'min':>10}{'max':>10}{'ext/base':>10}"]
    for L in [int(s) for s in args.sizes.split(",")]:
        log_n = L - LOG_B
        trace = zk.trace_fibsq((1 << log_n) - 1)
        for label, K, coset in (("K=3 coset leaves", 3, True), ("K=1 one-value leaves", 1, False)):
            ctxs = [zk.Context(log_n, LOG_B, fold_log=K, coset_leaves=coset, ext_log=e) for e in (0, 1)]
            times = [[], []]
            for c in ctxs:
                c.trace_upload(trace)
                for _ in range(3):
                    pr = c.prove()
            pr.verify(strict=True)                            # the ext context's last warm-up proof
            for _ in range(args.blocks):
                for e, c in enumerate(ctxs):
                    t0 = time.perf_counter()
                    for _ in range(args.proofs):
                        c.prove()
                    times[e].append((time.perf_counter() - t0) * 1e3 / args.proofs)
            med = [statistics.median(t) for t in times]
            for e in (0, 1):
                size = lib.zk_proof_data_len_ext(log_n, LOG_B, 1, 0, K, int(coset), 0, 0, e)
                lines.append(f"{label:<28}{'2^' + str(L):>8}{e:>5}{size:>13}{med[e]:>12.3f}{min(times[e]):>10.3f}{max(times[e]):>10.3f}{(f'{med[1] / med[0]:.2f}' if e else ''):>10}")
            for c in ctxs:
                c.close()
    lines += ["",
              f"# kernels on {name}: us per launch, median [min .. max] of {args.blocks} windows of {args.reps} launches",
              "# bytes: what the stage must move by count; GB/s: that count over the median (the same buffers every launch: cache-resident, not an HBM rate)",
              f"{'stage':<28}{'domain':>8}{'bytes':>14}{'median us':>12}{'min':>10}{'max':>10}{'GB/s':>9}{'ext/base':>10}"]

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps

    def pair(name, L, base, ext, base_bytes, ext_bytes):
        for fn in (base, ext):                               # warm-up: code objects loaded, tables and operands touched
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        tb, te = [], []
        for _ in range(args.blocks):
            tb.append(window(base))
            te.append(window(ext))
        mb, me = statistics.median(tb), statistics.median(te)
        for tag, t, m, nbytes, ratio in (("base", tb, mb, base_bytes, ""), ("ext", te, me, ext_bytes, f"{me / mb:.2f}")):
            lines.append(f"{name + ' ' + tag:<28}{'2^' + str(L):>8}{nbytes:>14}{m:>12.2f}{min(t):>10.2f}{max(t):>10.2f}{nbytes / m / 1e3:>9.1f}{ratio:>10}")

    for L in [int(s) for s in args.sizes.split(",")]:
        log_n, N = L - LOG_B, 1 << L
        dom = C.c_void_p()
        check(lib.zk_dom_create(0, log_n, LOG_B, 5, 0, C.byref(dom)))
        rng = np.random.default_rng(L)

        def up(n):
            return torch.from_numpy(rng.integers(0, P, n, dtype=np.uint32).view(np.int32)).to(dev)

        f, planes = up(N), up(2 * N)
        out = torch.empty(2 * N, dtype=torch.int32, device=dev)
        a3, a6, b2 = (C.c_uint32 * 3)(11, 22, 33), (C.c_uint32 * 6)(11, 12, 22, 23, 33, 34), (C.c_uint32 * 2)(77, 78)
        pair("compose", L,
             lambda: check(lib.zk_dev_compose(dom, f.data_ptr(), out.data_ptr(), 1, 2, a3, stream)),
             lambda: check(lib.zk_dev_compose_ext(dom, f.data_ptr(), out.data_ptr(), 1, 2, a6, stream)),
             8 * N, 12 * N)
        for steps in (1, 3):
            q = N >> steps
            pair(f"fold x{1 << steps}", L,
                 lambda: check(lib.zk_dev_fri_fold_multi(dom, planes.data_ptr(), out.data_ptr(), L, 0, steps, 77, stream)),
                 lambda: check(lib.zk_dev_fri_fold_multi_ext(dom, planes.data_ptr(), out.data_ptr(), L, 0, steps, b2, stream)),
                 4 * (N + q), 8 * (N + q))
        torch.cuda.synchronize()
        check(lib.zk_dom_destroy(dom))
        del f, planes, out
    report = "\n".join(lines) + "\n"
    sys.stdout.write(report)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(report)


if __name__ == "__main__":
    main()
