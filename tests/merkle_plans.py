"""The Merkle build planner (merkle_build_t, zkstark_amd/csrc/kernels.hip) restated in Python, for the tests.

plan() returns the launches a build runs and forms() the code paths inside them that the tree's levels take, so that a test
grid can be chosen to reach every path (tests/test_merkle_plans.py) and checked against the launches the library actually
profiles (tests/test_gpu_merkle_plans.py: a drifted mirror fails there, not silently).  The constants are the build's
defaults; each names the kernels.hip constant it mirrors, and each function the kernels.hip function it restates.
"""
import functools
from dataclasses import dataclass

# kernels.hip build-time constants (the defaults of a product build)
MAX_K = 4                  # ZK_MERKLE_MAX_K: levels per merkle_subtree_kernel launch
CHUNK_K = 3                # ZK_MERKLE_CHUNK_K: levels of a chunk build's one leaf launch
LATENCY_LOG = 17           # ZK_MERKLE_LATENCY_LOG: throughput launches while a level has more than 2^this nodes
FIELD_ROW_MAX = 16         # ZK_FIELD_ROW_MAX_NODES: field levels of <= this many nodes per workgroup use the 16-lane row form
FIELD_QUAD_MAX = 64        # ZK_FIELD_QUAD_MAX_NODES: ... of <= this many, the quad form
FIELD_ROW_LEAF_MAX = 32    # ZK_FIELD_ROW_LEAF_MAX: a workgroup with <= this many field leaves hashes them in the row form
WG_THREADS = 256           # kWgThreads: threads of a merkle_wg_kernel workgroup
WG_MAX_LOG = 10            # kWgMaxLog: levels of one merkle_wg_kernel phase, and nodes a continuation holds (2^10)
CONTINUE_US = 6.0          # kContinueUs
LAUNCH_US = 10.0           # kLaunchUs
CONTINUATION = True        # ZK_MERKLE_CONTINUATION
SHA, FIELD, B2S = 0, 1, 2  # hash_kind
# BLAKE2s one lane per hash: its instruction counts (csrc/kernels.hpp) times the time per instruction of the SHA-256 one-lane entries,
# in the operation order of kernels.hip -- the planner compares costs with a strict <, so the doubles must be the same bit for bit
B2S_INNER_OPS, SHA_INNER_OPS = 987.0, 2293.0        # kB2sInnerOps, kShaInnerOps
B2S_LEAF_OPS, SHA_LEAF_OPS = 954.0, 1259.0          # kB2sLeafOps, kShaLeafOps
B2S_LEVEL_US = B2S_INNER_OPS * 4.6 / SHA_INNER_OPS  # kB2sLevelUs
B2S_LEAF_US = B2S_LEAF_OPS * 2.6 / SHA_LEAF_OPS     # kB2sLeafUs


def wg_level_us(w, h):
    """wg_level_us: one workgroup's microseconds for a level of w nodes."""
    if w == 0:
        return 0.0
    if h == B2S:
        return float((w + 255) // 256) * B2S_LEVEL_US
    if h == FIELD:
        if w <= FIELD_ROW_MAX:
            return float((w + 15) // 16) * 3.7
        if w <= FIELD_QUAD_MAX:
            return float((w + 63) // 64) * 5.3
        return float((w + 255) // 256) * 10.8
    return 3.1 if w <= 64 else 4.9 if w <= 128 else float((w + 255) // 256) * 4.6


def wg_phase_us(leaf, cnt_log, levels, h, blocks):
    """wg_phase_us: the leaf hashes (or the first load) and `levels` levels of 2^cnt_log inputs, over `blocks` workgroups."""
    cnt = 1 << cnt_log
    if not leaf:
        us = 1.0
    elif h == FIELD:
        us = float((cnt + 15) // 16) * 3.7 if cnt <= FIELD_ROW_LEAF_MAX else float((cnt + 255) // 256) * 10.8
    else:
        us = float((cnt + 255) // 256) * (B2S_LEAF_US if h == B2S else 2.6)
    for t in range(1, levels + 1):
        us += wg_level_us(cnt >> t, h)
    return us * float(blocks) / 256.0 if blocks > 256 else us


def merkle_bytes(leaf, depth, k):
    """merkle_bytes: the algorithmic bytes a launch is profiled with."""
    n = float(1 << depth)
    produced = (n if leaf else 0.0) + n * (1.0 - 1.0 / float(1 << k))
    return (4.0 if leaf else 32.0) * n + 32.0 * produced


def chunk_handover_depth(log_m, log_chunks, lat):
    """chunk_handover_depth: the depth at which chunk builds stop and the finish pass starts."""
    if not (log_m > lat and lat >= log_chunks + 8):
        return log_chunks
    return log_m - min(log_m - lat, MAX_K, CHUNK_K)


@dataclass(frozen=True)
class Launch:
    kind: str          # "sub" (merkle_subtree_kernel) or "wg" (merkle_wg_kernel)
    leaf: bool         # reads the leaves through the source
    depth: int         # depth_in: the absolute depth of the launch's inputs
    span: int          # depth_in - stop: inputs of the launch are 2^span
    k: int             # sub: levels; wg: j, the levels of phase 0
    j2: int = 0        # wg: levels of the continuation (phase 1)

    @property
    def cls(self):
        """The kernel class of the profiler (ScopedKernelTimer in merkle_build_t)."""
        return ("merkle_leaf" if self.leaf else "merkle_inner") if self.kind == "sub" else "merkle_top"

    @property
    def bytes(self):
        if self.kind == "sub":
            return merkle_bytes(self.leaf, self.span, self.k)
        return merkle_bytes(self.leaf, self.span, self.k) + (merkle_bytes(False, self.span - self.k, self.j2) if self.j2 else 0.0)


def plan(log_m, h, counter=False, top=0, lat=LATENCY_LOG, log_sub=None, chunk=0, leaf_mode=True, tp_floor=0):
    """merkle_build_t(src, log_m, mail{counter, top}, hash, log_sub, chunk, leaf_mode, tp_floor) -> [Launch]."""
    if log_sub is None:
        log_sub = log_m
    stop = log_m - log_sub
    depth, leaf = log_m, leaf_mode
    out = []
    floor_depth = tp_floor if tp_floor else stop + lat
    while depth > floor_depth:
        k = min(depth - floor_depth, MAX_K)
        out.append(Launch("sub", leaf, depth, depth - stop, k))
        leaf, depth = False, depth - k
    if tp_floor:
        return out
    if stop != 0 or top >= log_m:
        top = 0
    end = top if stop == 0 else stop
    may_continue = stop == 0 and counter and CONTINUATION
    while True:
        span, levels = depth - stop, depth - end
        launches = (levels + WG_MAX_LOG - 1) // WG_MAX_LOG if levels else 1
        jn = (levels + launches - 1) // launches
        best_j, best_j2 = jn, 0
        if may_continue and levels <= 2 * WG_MAX_LOG:
            best = wg_phase_us(leaf, jn, jn, h, 1 << (span - jn))
            if launches == 2 and span - jn <= WG_MAX_LOG:
                best += LAUNCH_US + wg_phase_us(False, span - jn, levels - jn, h, 1)
            elif launches > 1:
                best = 0.0
            for j in range(1, min(levels - 1, WG_MAX_LOG) + 1):
                j2 = levels - j
                if j2 > WG_MAX_LOG or span - j > WG_MAX_LOG:
                    continue
                us = wg_phase_us(leaf, j, j, h, 1 << (span - j)) + CONTINUE_US + wg_phase_us(False, span - j, j2, h, 1)
                if us < best:
                    best, best_j, best_j2 = us, j, j2
        out.append(Launch("wg", leaf, depth, span, best_j, best_j2))
        leaf, depth = False, depth - best_j - best_j2
        if depth <= end:
            return out


def chunk_plans(log_m, log_chunks, h, lat=LATENCY_LOG, counter=False, top=0):
    """zk_dev_merkle_build_chunk for every chunk, then zk_dev_merkle_finish (counter=False) or zk_dev_merkle_commit_finish."""
    log_sub = log_m - log_chunks
    hd = chunk_handover_depth(log_m, log_chunks, lat)
    chunks = [plan(log_m, h, lat=lat, log_sub=log_sub, chunk=c, tp_floor=hd if hd != log_chunks else 0)
              for c in range(1 << log_chunks)]
    start = chunk_handover_depth(log_m, log_chunks, lat)
    if start == 0:
        return chunks, []
    if top and start <= top:
        top = 0
    return chunks, plan(start, h, counter=counter, top=top, lat=lat, leaf_mode=False)


def level_form(w, h):
    """The form merkle_wg_kernel hashes a level of w nodes per workgroup in.  BLAKE2s has the one-lane form only; "lane2" names
    its levels of more than 256 nodes per workgroup, where a thread hashes two nodes (a1 in the kernel)."""
    if h == B2S:
        return "lane2" if w > WG_THREADS else "lane"
    if h == FIELD:
        return "row" if w <= FIELD_ROW_MAX else "quad" if w <= FIELD_QUAD_MAX else "lane"
    return "quad" if w <= 64 else "split" if w <= 128 else "lane"


def forms(launches, h):
    """The code paths the launches take: ("sub", "leaf" | "inner", k), ("leaf", "row" | "lane") for the leaf hashes of a
    merkle_wg_kernel launch, and (phase, form) for every level it hashes (phase 1: the continuation).  BLAKE2s, whose levels
    have one form, also names the edges of the lane path: ("leaf", "lane4") for a leaf phase of more than 256 leaves per
    workgroup (a thread keeps several fetched inputs: kPer > 1 in use), and ("load", phase, "one" | "many") for the first load
    of an inner-mode launch (phase 0) and of the continuation (phase 1) of at most / more than 256 digests."""
    fs = set()
    for la in launches:
        if la.kind == "sub":
            fs.add(("sub", "leaf" if la.leaf else "inner", la.k))
            continue
        cnt = 1 << la.k
        if la.leaf:
            if h == B2S:
                fs.add(("leaf", "lane4" if cnt > WG_THREADS else "lane"))
            else:
                fs.add(("leaf", "row" if h == FIELD and cnt <= FIELD_ROW_LEAF_MAX else "lane"))
        elif h == B2S:
            fs.add(("load", 0, "many" if cnt > WG_THREADS else "one"))
        if h == B2S and la.j2:
            fs.add(("load", 1, "many" if (1 << (la.span - la.k)) > WG_THREADS else "one"))
        for t in range(1, la.k + 1):
            fs.add((0, level_form(cnt >> t, h)))
        for t in range(1, la.j2 + 1):
            fs.add((1, level_form((1 << (la.span - la.k)) >> t, h)))
    return fs


def profile(launches):
    """{class: (launches, bytes)} as zk_dev_kernel_stats reports them for these launches."""
    out = {}
    for la in launches:
        n, b = out.get(la.cls, (0, 0.0))
        out[la.cls] = (n + 1, b + la.bytes)
    return out


# ---- the grid of tests/test_gpu_merkle_plans.py ---------------------------------------------------------------------------
MAX_LOG = {SHA: 22, FIELD: 20, B2S: 20}   # largest tree per hash
LATS = range(17, 11, -1)             # zk_dev_set_merkle_latency_log values the grid sweeps (the default first)
TOPS = (0, 1, 3, 8)                  # committer hand-over depths (zk_committer_set_top; SHA-256 only)


def _wg_shape(launches):
    return tuple((la.leaf, la.span, la.k, la.j2) for la in launches if la.kind == "wg")


def latency_shapes(h, counter, top=0, leaf_mode=True):
    """The smallest (log_m, lat) for every distinct latency phase (the merkle_wg_kernel launches, their (j, j2) splits and
    whether they hash the leaves) that trees up to MAX_LOG[h] leaves reach for lat in LATS."""
    seen = {}
    for log_m in range(MAX_LOG[h] + 1):
        for lat in LATS:
            shape = _wg_shape(plan(log_m, h, counter, top, lat, leaf_mode=leaf_mode))
            seen.setdefault((shape, min(top, log_m) if top < log_m else 0), (log_m, lat))
    return sorted(seen.values())


# throughput launches: a leaf launch of k = 1, 2, 3 levels (log_m - lat = k), and k = 4 followed by inner launches of 1 .. 4
THROUGHPUT_SHAPES = [(12 + d, 12) for d in (1, 2, 3, 5, 6, 7, 8)]


def build_cases(h):
    """zk_dev_merkle_build_ex (no counter: phase 0 only): (log_m, lat)."""
    return sorted(set(latency_shapes(h, False)) | set(THROUGHPUT_SHAPES))


def commit_cases(h):
    """zk_dev_merkle_commit (a counter: the continuation): (log_m, lat, top, log_parts)."""
    out = set()
    for top in (TOPS if h == SHA else (0,)):
        out |= {(log_m, lat, top, 0) for log_m, lat in latency_shapes(h, True, top)}
    out.add((MAX_LOG[h], 17, 0, 0))                   # the largest tree, as a proof commits it
    if h == SHA:
        out.add((MAX_LOG[h], 17, 8, 0))
        out.add((19, 19, 0, 0))                       # the one-lane SHA-256 form in the continuation (j = 10, j2 = 9)
    # leaves in all-to-all order (InterleaveSrc): the leaf row / lane forms, a throughput leaf launch, a continuation
    out |= {(5, 17, 0, 2), (11, 17, 0, 3), (16, 12, 0, 1), (18, 15, 0, 4)}
    if h == SHA:
        out |= {(11, 17, 3, 3), (16, 12, 8, 1)}
    return sorted(out)


def context_cases(h):
    """Whole trees with a counter that only a context builds (BLAKE2s: zk_dev_merkle_commit refuses the hash), through
    Context.merkle_commit(0): (log_m, lat).  The smallest context has a layer 0 of 2^3 values; the smaller trees with a counter
    are the last FRI trees of a proof (tests/test_gpu_merkle_plans.py: the context trees after a second trace)."""
    return [(log_m, lat) for log_m, lat in latency_shapes(h, True) if log_m >= 3]


def coset_cases(h):
    """Trees with coset leaves through Context.merkle_commit(0, coset_steps): one coset_leaf_hash_kernel launch, then the
    inner-mode build with a counter: (steps, log_m, lat) for a tree of 2^log_m leaves over 2^(log_m + steps) values.  Every
    latency phase of inner mode, and below a switch at 2^12 an inner throughput launch of k = 1 .. 4 levels; every steps in
    both groups."""
    out = {(1 + log_m % 3, log_m, lat) for log_m, lat in latency_shapes(h, True, leaf_mode=False) if log_m >= 1}
    out |= {(1, 13, 12), (2, 14, 12), (3, 15, 12), (2, 16, 12)}
    return sorted(out)


def chunk_cases(h):
    """zk_dev_merkle_build_chunk for every chunk, then the finish pass: (log_m, log_chunks, lat, log_parts, top); top None =
    zk_dev_merkle_finish, else zk_dev_merkle_commit_finish with that committer top."""
    out = [
        (4, 4, 17, 0, None),     # one leaf per chunk
        (6, 1, 17, 1, None),     # chunks built to their roots by merkle_wg_kernel (off != 0), then a 2-leaf finish
        (10, 2, 17, 2, 0),
        (14, 5, 12, 3, None),    # lat < log_chunks + 8: the chunks still go to their roots
        (14, 2, 12, 1, None),    # throughput-only chunks (k = 2) and a finish over 2^12 nodes
        (16, 1, 12, 2, 0),       # k = 3 chunks, the finish runs a throughput launch first, with a continuation
        (18, 4, 13, 2, None),
    ]
    if h == SHA:
        out += [(10, 2, 17, 2, 8), (16, 1, 12, 2, 3), (18, 4, 13, 2, 8)]
    return out


# BLAKE2s forms that no latency log of LATS reaches: the smallest whole tree with a counter at a raised log for each
# (tests/test_merkle_plans.py names them)
B2S_RAISED_CASES = [(19, 19), (20, 20)]


def chunk_launches(h, log_m, log_chunks, lat, top):
    chunks, fin = chunk_plans(log_m, log_chunks, h, lat, counter=top is not None, top=top or 0)
    return [la for c in chunks for la in c] + fin


def grid_forms(h):
    """Every form the grid above reaches for hash h."""
    fs = set()
    for log_m, lat in build_cases(h):
        fs |= forms(plan(log_m, h, False, 0, lat), h)
    if h == B2S:                                          # no committer and no chunks for this hash: the context grids instead
        for log_m, lat in context_cases(h) + B2S_RAISED_CASES:
            fs |= forms(plan(log_m, h, True, 0, lat), h)
        for _, log_m, lat in coset_cases(h):
            fs |= forms(plan(log_m, h, True, 0, lat, leaf_mode=False), h)
        return fs
    for log_m, lat, top, _ in commit_cases(h):
        fs |= forms(plan(log_m, h, True, top, lat), h)
    for log_m, lc, lat, _, top in chunk_cases(h):
        fs |= forms(chunk_launches(h, log_m, lc, lat, top), h)
    return fs


@functools.lru_cache(maxsize=None)
def all_forms(h, lats=range(12, 25)):
    """Every form the planner reaches for hash h: whole trees of 2^0 .. 2^30 leaves with and without a counter, every committer
    top, every latency log the library accepts, and chunked builds.  BLAKE2s has neither tops nor chunks: whole trees with and
    without a counter, from the leaves and (below a coset-leaf launch) in inner mode."""
    fs = set()
    if h == B2S:
        for log_m in range(31):
            for lat in lats:
                for counter in (False, True):
                    for leaf_mode in (True, False):
                        fs |= forms(plan(log_m, h, counter, 0, lat, leaf_mode=leaf_mode), h)
        return fs
    for log_m in range(31):
        for lat in lats:
            for counter in (False, True):
                for top in (TOPS if h == SHA and counter else (0,)):
                    fs |= forms(plan(log_m, h, counter, top, lat), h)
            for lc in range(0, min(log_m, 10) + 1):
                fs |= forms(chunk_launches(h, log_m, lc, lat, None), h)
    return fs
