// grind.hip -- proof-of-work grinding before the query draw (DESIGN.md "Grinding"; the reference has none).
//
// The search: the smallest nonce w >= start such that SHA-256(S || le64(w)) begins with g zero bits, S the 32-byte channel
// state after the free term.  The message is one block: W0..7 = S, W8 = bswap(lo32 w), W9 = bswap(hi32 w), W10 = 0x80000000,
// W11..14 = 0, W15 = 320.  On the device:
//   * rounds 0..7 see only S: the host passes the state after round 7 (the midstate) and the kernel starts at round 8;
//   * a launch never crosses a multiple of 2^32, so W9 is uniform within it and only W8 varies per lane: the host passes
//     W16..W22 (which do not depend on W8) and the kernel computes the schedule from W23 on;
//   * only digest word 0 is formed (the compiler drops what it does not feed);
//   * one lane per nonce, several nonces per lane in increasing order over the whole grid; a wave with a hit posts its
//     smallest one with ONE 64-bit device-scope atomicMin, and a wave stops once its next nonce exceeds the current best.
// The host searches [start, start + chunk) in increasing chunks and stops after the first chunk with a hit, so the result is
// the smallest nonce.  Results reach the host through a pinned, device-mapped mailbox the last workgroup fills and flags (the
// pattern of the prover's openings, zkstark.hip open_launch / open_wait): no stream synchronisation, no copy command.
// One launch grinds for many proofs at once (the batch prover): grid = nonce blocks x jobs, each job its own midstate and
// best word; a job's search ends on its own and only the unfinished ones are launched again.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "internal.hpp"
#include "sha256.hpp"
#include "transcript.hpp"

using namespace zk;
using namespace zk::impl;

namespace zk {
namespace {

constexpr uint32_t kGrindThreads = 256;
constexpr uint64_t kGrindMinChunk = (uint64_t)1 << 14;
constexpr uint64_t kGrindMaxChunk = (uint64_t)1 << 32;
constexpr uint64_t kNoNonce = ~(uint64_t)0;

struct GrindJob {
    uint32_t mid[8];          // a .. h after rounds 0..7
    uint32_t w[23];           // schedule words 0..22 with W8 = 0 (W9 = bswap(hi32) of this launch)
    uint32_t slot;            // this job's best word and mailbox slot
};
struct GrindArgs {
    const GrindJob* jobs;     // host-mapped, [gridDim.y]
    unsigned long long* best; // device, [slots]: ~0 = no hit yet; posted and reset by the last workgroup
    uint32_t* mailbox;        // host-mapped: word 0 = seq, then one u64 per slot from word 2
    uint32_t* counter;        // one zeroed device word: workgroups done
    uint64_t start;           // first nonce of the launch
    uint64_t count;           // nonces per job, <= 2^32 (start .. start + count - 1 share hi32)
    uint32_t mask;            // hit: (digest word 0 & mask) == 0
    uint32_t seq;
};

#define GR_ROUND(i, wi)                                                                        \
    do {                                                                                       \
        const uint32_t S1 = sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25));        \
        const uint32_t t1 = (h + S1 + sha_ch(e, f, g)) + (SHA_K[i] + (wi));                    \
        const uint32_t S0 = sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22));        \
        const uint32_t mj = sha_maj(a, b, c);                                                  \
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;                \
    } while (0)

// Digest word 0 of the block for one value of W8 (rounds 8..63 from the midstate).
__device__ __forceinline__ uint32_t grind_word(const uint32_t (&mid)[8], const uint32_t (&wu)[23], uint32_t w8) {
    uint32_t W[64];
#pragma unroll
    for (int i = 0; i < 23; ++i) W[i] = wu[i];
    W[8] = w8;
#pragma unroll
    for (int t = 23; t < 64; ++t) {
        const uint32_t w15 = W[t - 15], w2 = W[t - 2];
        const uint32_t s0 = sha_xor3(sha_rotr(w15, 7), sha_rotr(w15, 18), w15 >> 3);
        const uint32_t s1 = sha_xor3(sha_rotr(w2, 17), sha_rotr(w2, 19), w2 >> 10);
        W[t] = (W[t - 16] + s0 + W[t - 7]) + s1;
    }
    uint32_t a = mid[0], b = mid[1], c = mid[2], d = mid[3], e = mid[4], f = mid[5], g = mid[6], h = mid[7];
#pragma unroll
    for (int i = 8; i < 64; ++i) GR_ROUND(i, W[i]);
    return SHA_IV[0] + a;
}

__global__ void __launch_bounds__(kGrindThreads) grind_kernel(GrindArgs a) {
    const GrindJob& jb = a.jobs[blockIdx.y];
    const uint32_t slot = jb.slot;
    uint32_t mid[8], wu[23];
#pragma unroll
    for (int i = 0; i < 8; ++i) mid[i] = jb.mid[i];
#pragma unroll
    for (int i = 0; i < 23; ++i) wu[i] = jb.w[i];
    const uint64_t lanes = (uint64_t)gridDim.x * kGrindThreads;
    const uint32_t lane = blockIdx.x * kGrindThreads + threadIdx.x;
    const uint32_t wave_first = lane & ~63u;
    const uint32_t lo0 = (uint32_t)a.start;
    for (uint64_t base = 0; base < a.count; base += lanes) {
        if (base) {                                       // every nonce left to this wave is above the best hit: done
            const unsigned long long bst = __hip_atomic_load(&a.best[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a.start + base + wave_first > bst) break;
        }
        const uint64_t idx = base + lane;
        const uint32_t d0 = grind_word(mid, wu, __builtin_bswap32(lo0 + (uint32_t)idx));
        const bool hit = idx < a.count && (d0 & a.mask) == 0u;
        const unsigned long long m = __ballot(hit);
        if (m) {                                          // the wave's smallest hit: its lowest lane
            if ((threadIdx.x & 63u) == (uint32_t)(__ffsll(m) - 1))
                __hip_atomic_fetch_min(&a.best[slot], (unsigned long long)(a.start + idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
    // the workgroup that finishes last posts every job's best word to the mailbox, resets it, and raises the flag
    __threadfence();
    __syncthreads();
    __shared__ uint32_t is_last;
    if (threadIdx.x == 0) {
        const uint32_t total = gridDim.x * gridDim.y;
        const uint32_t done = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = done == total - 1u;
        if (is_last) __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    for (uint32_t j = threadIdx.x; j < gridDim.y; j += kGrindThreads) {
        const uint32_t s = a.jobs[j].slot;
        const unsigned long long v = __hip_atomic_exchange(&a.best[s], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.mailbox[2 + 2 * s] = (uint32_t)v;
        a.mailbox[3 + 2 * s] = (uint32_t)(v >> 32);
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&a.mailbox[0], a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The job of one state for the launches whose nonces share hi32 = hi.
void make_job(const uint8_t S[32], uint32_t hi, uint32_t slot, GrindJob& j) {
    uint32_t W[23] = {0};
    for (int i = 0; i < 8; ++i) W[i] = ((uint32_t)S[4 * i] << 24) | ((uint32_t)S[4 * i + 1] << 16) | ((uint32_t)S[4 * i + 2] << 8) | S[4 * i + 3];
    W[9] = __builtin_bswap32(hi);
    W[10] = 0x80000000u;
    W[15] = 320u;
    for (int t = 16; t < 23; ++t) {                       // W8 first enters at t = 23 (s0(W[t - 15]))
        const uint32_t w15 = W[t - 15], w2 = W[t - 2];
        W[t] = W[t - 16] + sha_xor3(sha_rotr(w15, 7), sha_rotr(w15, 18), w15 >> 3) + W[t - 7] + sha_xor3(sha_rotr(w2, 17), sha_rotr(w2, 19), w2 >> 10);
    }
    uint32_t a = SHA_IV[0], b = SHA_IV[1], c = SHA_IV[2], d = SHA_IV[3], e = SHA_IV[4], f = SHA_IV[5], g = SHA_IV[6], h = SHA_IV[7];
    for (int i = 0; i < 8; ++i) GR_ROUND(i, W[i]);
    const uint32_t st[8] = {a, b, c, d, e, f, g, h};
    memcpy(j.mid, st, sizeof st);
    memcpy(j.w, W, sizeof W);
    j.slot = slot;
}

uint32_t grind_mask(uint32_t bits) { return bits ? ~0u << (32 - bits) : 0u; }

}  // namespace

namespace impl {

struct Grinder {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t max_jobs = 0, blocks = 0;
    GrindJob* h_jobs = nullptr;                 // pinned, device-mapped
    GrindJob* dm_jobs = nullptr;
    uint32_t* h_mail = nullptr;                 // pinned, coherent, device-mapped
    uint32_t* dm_mail = nullptr;
    unsigned long long* d_best = nullptr;       // [max_jobs]
    uint32_t* d_counter = nullptr;
    uint32_t seq = 0;
    bool dirty = false;                         // a launch was waited for in vain: best words and counter are reset first
};

void grinder_destroy(Grinder* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->h_jobs) (void)hipHostFree(g->h_jobs);
    if (g->h_mail) (void)hipHostFree(g->h_mail);
    if (g->d_best) (void)hipFree(g->d_best);
    if (g->d_counter) (void)hipFree(g->d_counter);
    if (g->own_stream && g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

int grinder_create(int device, void* stream, uint32_t max_jobs, Grinder** out) {
    *out = nullptr;
    if (max_jobs < 1 || max_jobs > 65535) return fail(ZK_ERR_INVALID, "grinder: need 1 <= jobs <= 65535");
    HIPCHK(hipSetDevice(device));
    Grinder* g = new (std::nothrow) Grinder();
    if (!g) return fail(ZK_ERR_NOMEM, "out of host memory");
    g->device = device;
    g->max_jobs = max_jobs;
    int cus = 0;
    // exactly the workgroups that are resident at once: every lane then walks the nonces in step with the others, and no
    // workgroup that starts late sweeps the low nonces after the rest have passed them (the search would end with it)
    int per_cu = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(grind_kernel), kGrindThreads, 0);
    g->blocks = (uint32_t)std::max(1, cus) * (uint32_t)std::max(1, per_cu);
    if (e == hipSuccess) {
        if (stream) g->stream = (hipStream_t)stream;
        else { e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking); g->own_stream = e == hipSuccess; }
    }
    if (e == hipSuccess) e = hipHostMalloc((void**)&g->h_jobs, sizeof(GrindJob) * max_jobs, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&g->dm_jobs, g->h_jobs, 0);
    if (e == hipSuccess) e = hipHostMalloc((void**)&g->h_mail, 8 + 8 * (size_t)max_jobs, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&g->dm_mail, g->h_mail, 0);
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_best, 8 * (size_t)max_jobs);
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_counter, 64);
    if (e == hipSuccess) e = hipMemsetAsync(g->d_best, 0xff, 8 * (size_t)max_jobs, g->stream);
    if (e == hipSuccess) e = hipMemsetAsync(g->d_counter, 0, 64, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) {
        grinder_destroy(g);
        return fail(ZK_ERR_HIP, "grinder: %s", hipGetErrorString(e));
    }
    memset(g->h_mail, 0, 8 + 8 * (size_t)max_jobs);
    *out = g;
    return ZK_OK;
}

// First chunk: about 4 * 2^g nonces, so that one launch finds a hit with probability 1 - e^-4 ~ 98 %.
uint64_t grind_chunk(uint32_t bits) {
    const uint64_t c = bits >= 31 ? kGrindMaxChunk : (uint64_t)4 << bits;
    return std::min(std::max(c, kGrindMinChunk), kGrindMaxChunk);
}

int grind_device(Grinder* g, const uint8_t* states, size_t count, uint32_t bits, uint64_t start, uint64_t* nonces_out) {
    if (!g || (count && (!states || !nonces_out))) return fail(ZK_ERR_INVALID, "grind: null argument");
    if (bits > kMaxGrindBits) return fail(ZK_ERR_INVALID, "grind: need grind_bits <= %u (got %u)", kMaxGrindBits, bits);
    if (count > g->max_jobs) return fail(ZK_ERR_INVALID, "grind: %zu states, the grinder holds %u", count, g->max_jobs);
    if (start > ~(uint64_t)0 - kGrindLimit) return fail(ZK_ERR_INVALID, "grind: start + 2^44 overflows");
    if (bits == 0) { for (size_t i = 0; i < count; ++i) nonces_out[i] = start; return ZK_OK; }
    HIPCHK(hipSetDevice(g->device));
    if (g->dirty) {
        HIPCHK(hipMemsetAsync(g->d_best, 0xff, 8 * (size_t)g->max_jobs, g->stream));
        HIPCHK(hipMemsetAsync(g->d_counter, 0, 64, g->stream));
        g->dirty = false;
    }
    std::vector<uint32_t> active(count);
    for (size_t i = 0; i < count; ++i) active[i] = (uint32_t)i;
    const uint64_t chunk = grind_chunk(bits);
    uint64_t pos = start;
    uint32_t job_hi = 0;
    bool jobs_valid = false;
    while (!active.empty()) {
        if (pos - start >= kGrindLimit)
            return fail(ZK_ERR_HIP, "grind: no nonce with %u leading zero bits among 2^44 nonces from %llu", bits, (unsigned long long)start);
        const uint64_t to_carry = ((uint64_t)1 << 32) - (pos & 0xFFFFFFFFu);
        const uint64_t n = std::min(chunk, to_carry);
        const uint32_t hi = (uint32_t)(pos >> 32);
        if (!jobs_valid || hi != job_hi) {                // W9 and the schedule words after it change with hi32
            for (size_t j = 0; j < active.size(); ++j) make_job(states + 32 * (size_t)active[j], hi, active[j], g->h_jobs[j]);
            job_hi = hi;
            jobs_valid = true;
        }
        GrindArgs a;
        a.jobs = g->dm_jobs; a.best = g->d_best; a.mailbox = g->dm_mail; a.counter = g->d_counter;
        a.start = pos; a.count = n; a.mask = grind_mask(bits); a.seq = ++g->seq;
        uint64_t bx = (a.count + kGrindThreads - 1) / kGrindThreads;
        const uint64_t per_job = std::max<uint64_t>(1, g->blocks / active.size());
        if (bx > per_job) bx = per_job;
        hipLaunchKernelGGL(grind_kernel, dim3((uint32_t)bx, (uint32_t)active.size()), dim3(kGrindThreads), 0, g->stream, a);
        HIPCHK(hipGetLastError());
        if (int rc = wait_flag(g->h_mail, a.seq, g->stream)) { g->dirty = true; return rc; }
        std::vector<uint32_t> still;
        size_t kept = 0;
        for (size_t j = 0; j < active.size(); ++j) {
            const uint32_t s = active[j];
            const uint64_t v = (uint64_t)g->h_mail[2 + 2 * s] | ((uint64_t)g->h_mail[3 + 2 * s] << 32);
            if (v != kNoNonce) nonces_out[s] = v;
            else { still.push_back(s); if (kept != j) g->h_jobs[kept] = g->h_jobs[j]; ++kept; }
        }
        active.swap(still);
        pos += n;
    }
    return ZK_OK;
}

// The same search on `threads` host threads (1: the calling thread alone).  Thread t takes the blocks t, t + T, t + 2T, ... of
// kBlk nonces in increasing order and stops at its first hit or once its next block starts above the best hit so far, so
// every nonce below the result has been tested.
int grind_host(const uint8_t state[32], uint32_t bits, uint64_t start, uint32_t threads, uint64_t* nonce_out) {
    if (!state || !nonce_out) return fail(ZK_ERR_INVALID, "zk_grind_host: null argument");
    if (bits > kMaxGrindBits) return fail(ZK_ERR_INVALID, "zk_grind_host: need grind_bits <= %u (got %u)", kMaxGrindBits, bits);
    if (start > ~(uint64_t)0 - kGrindLimit) return fail(ZK_ERR_INVALID, "zk_grind_host: start + 2^44 overflows");
    if (bits == 0) { *nonce_out = start; return ZK_OK; }
    const uint32_t T = std::min<uint32_t>(std::max<uint32_t>(threads, 1), 16);
    constexpr uint64_t kBlk = 1024;
    uint32_t tmpl[16] = {0};
    for (int i = 0; i < 8; ++i)
        tmpl[i] = ((uint32_t)state[4 * i] << 24) | ((uint32_t)state[4 * i + 1] << 16) | ((uint32_t)state[4 * i + 2] << 8) | state[4 * i + 3];
    tmpl[10] = 0x80000000u;
    tmpl[15] = 320u;
    const uint32_t mask = grind_mask(bits);
    std::atomic<uint64_t> best{kNoNonce};
    auto worker = [&](uint32_t t) {
        uint32_t blk[16];
        memcpy(blk, tmpl, sizeof blk);
        for (uint64_t k = t;; k += T) {
            const uint64_t off = k * kBlk;
            if (off >= kGrindLimit) return;
            const uint64_t b0 = start + off;
            if (b0 > best.load(std::memory_order_relaxed)) return;
            for (uint64_t w = b0; w < b0 + kBlk; ++w) {
                blk[8] = __builtin_bswap32((uint32_t)w);
                blk[9] = __builtin_bswap32((uint32_t)(w >> 32));
                uint32_t st[8];
                memcpy(st, SHA_IV, sizeof st);
                host_sha_compress(st, blk);
                if ((st[0] & mask) == 0) {
                    uint64_t cur = best.load(std::memory_order_relaxed);
                    while (w < cur && !best.compare_exchange_weak(cur, w, std::memory_order_relaxed)) {}
                    return;
                }
            }
        }
    };
    if (T == 1) worker(0);
    else {
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < T; ++t) th.emplace_back(worker, t);
        worker(0);
        for (auto& x : th) x.join();
    }
    const uint64_t b = best.load();
    if (b == kNoNonce) return fail(ZK_ERR_HIP, "zk_grind_host: no nonce with %u leading zero bits among 2^44 nonces from %llu", bits, (unsigned long long)start);
    *nonce_out = b;
    return ZK_OK;
}

// The prover's step: the nonce for the channel's state (host below the threshold, else the device), committed to the channel.
int grind_channel(Grinder* g, Channel& ch, uint32_t bits, uint64_t* nonce_out) {
    uint64_t w = 0;
    int rc = (bits <= kGrindHostMaxBits || !g) ? grind_host(ch.state, bits, 0, 1, &w) : grind_device(g, ch.state, 1, bits, 0, &w);
    if (rc) return rc;
    grind_commit(ch, w);
    *nonce_out = w;
    return ZK_OK;
}

}  // namespace impl
}  // namespace zk

namespace {
std::mutex g_dev_grinders_mu;
Grinder* g_dev_grinders[64] = {nullptr};   // zk_grind: one per device, on a stream of its own (never freed: process lifetime)
}  // namespace

extern "C" {

int zk_grind(int device, const uint8_t state[32], uint32_t grind_bits, uint64_t start, uint64_t* nonce_out) {
    if (!state || !nonce_out) return fail(ZK_ERR_INVALID, "zk_grind: null argument");
    if (grind_bits > kMaxGrindBits) return fail(ZK_ERR_INVALID, "zk_grind: need grind_bits <= %u (got %u)", kMaxGrindBits, grind_bits);
    if (device < 0 || device >= 64) return fail(ZK_ERR_INVALID, "zk_grind: device %d out of range", device);
    std::lock_guard<std::mutex> lk(g_dev_grinders_mu);
    if (!g_dev_grinders[device])
        if (int rc = grinder_create(device, nullptr, 1, &g_dev_grinders[device])) return rc;
    return grind_device(g_dev_grinders[device], state, 1, grind_bits, start, nonce_out);
}

int zk_grind_host(const uint8_t state[32], uint32_t grind_bits, uint64_t start, uint32_t threads, uint64_t* nonce_out) {
    return grind_host(state, grind_bits, start, threads, nonce_out);
}

}  // extern "C"
